// melspec.hip -- spectrogram / melspectrogram / mfcc / welch_pgram (DSP.spectrogram, DSP.welch_pgram + src/mel.jl) on gfx950: one STFT
// engine, four epilogues.
//
// Frames are DSP.arraysplit's (k = (L-n) / (n-noverlap) + 1), windowed and zero-padded to nfft.  Two real frames travel as one complex
// sequence z = a + i b (frame 2p real, frame 2p+1 imaginary); after the FFT X_a[k] = (Z_k + conj Z_{N-k}) / 2 and
// X_b[k] = (Z_k - conj Z_{N-k}) / (2i).  The signal is read in place at the frame offsets (no frame matrix).
//   * 7-smooth nfft <= 8192: B frame pairs per workgroup, a Stockham mixed-radix FFT (8/4/2/3/5/7) in one 128 KiB LDS buffer, the
//     split, the power, then the epilogue from LDS: power rows, mel bands (each a contiguous-range sum in bin order), or the DCT and
//     column norm of the MFCC.  Only the final output reaches HBM.
//   * 7-smooth nfft > 8192 (<= 2^26): four-step, nfft = n1 n2 with both factors <= 8192: the LDS FFT on the columns (times the twiddle
//     w^(j2 k1), built from two tables), then on the rows, global scratch in between; split + power; epilogue from the power columns.
//   * any other nfft: Bluestein on a 7-smooth m >= 2 nfft - 1 through the same FFT (in LDS when m <= 8192, else four-step).  The chirp
//     exp(-i pi k^2 / nfft) is reduced as k^2 mod 2 nfft in 64-bit integers before the table lookup.
// Twiddles come from host tables with exact argument reduction (octant, long double).  All device arithmetic is double, products are
// rounded (-ffp-contract=off), and nothing is accumulated by atomics: the outputs are bitwise reproducible.
// The fourth epilogue (LPVS_STFT_WELCH) is the mean of the power over the frames.  On the LDS paths workgroup g of S adds the power
// columns of its batch (in LDS, never a power matrix in HBM) in ascending frame order to slab g of nbins partial sums; batch g + S, g + 2 S, ...
// follow in further launches of the same S workgroups, so a slab is only ever touched by one workgroup at a time, in frame order.  (One
// launch whose workgroups loop over their batches with the sums in LDS was measured at 3x the time: the FFT already fills the register
// file, and the loop's live state spills.)  On the four-step paths a chunk's spectra already sit in global scratch: the split, the power
// and the sum over slabs of kWelchChunkFrames frames are one kernel, a thread per bin.
// A second kernel adds the slabs in a fixed pairwise tree and a third divides by the frame count.  The longest chain of dependent
// additions behind one bin is D = F - 1 + ceil(log2 S), F the most frames behind one slab (<= kWelchChain), S the slabs.
#include "lpvs_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace lpvs {
namespace {

constexpr int kFftMax = 8192;        // complex points per workgroup (16 B each: 128 KiB of LDS)
constexpr int kThreads = 512;           // 8 waves: up to 256 VGPRs each, no spills in the radix-7 stage
constexpr int kMaxStages = 16;
constexpr int kMaxPairs = 512;       // frame pairs per workgroup (small nfft)
constexpr int kSplitPer = 10;        // split items per thread: pairs x bins of a workgroup <= kSplitPer * kThreads (host-checked)
constexpr int64_t kMaxLen = 1ll << 26;
constexpr int64_t kRootB = 8192;     // two-table roots: r = hi * kRootB + lo
constexpr int kEpiThreads = 256;
constexpr size_t kScratchBudget = (size_t)1 << 30;   // bytes of four-step scratch per chunk of frame pairs
constexpr int64_t kWelchChain = 1024;        // most frames one workgroup adds sequentially into its slab (LDS paths)
constexpr int64_t kWelchSlabs = 1024;        // slabs launched when the frames allow it (more when kWelchChain asks for it)
constexpr int64_t kWelchChunkFrames = 256;   // frames per slab on the four-step paths

enum : int { IN_SIGNAL = 0, IN_GLOBAL = 1 };
enum : int { POST_NONE = 0, POST_TWIDDLE = 1, POST_BLUE_MUL = 2, POST_BLUESTEIN_LDS = 3 };
enum : int { OUT_GLOBAL = 0, OUT_EPI = 1 };

__host__ __device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline double2 conjd(double2 a) { return make_double2(a.x, -a.y); }

// ---- host: 7-smooth lengths, factorisation, roots -----------------------------------------------------------------------------------
bool is_smooth(int64_t n) {
    if (n < 1) return false;
    for (int64_t p : {2, 3, 5, 7}) while (n % p == 0) n /= p;
    return n == 1;
}
int64_t next_smooth(int64_t n) {
    int64_t m = n < 1 ? 1 : n;
    while (!is_smooth(m)) ++m;
    return m;
}
struct Radices { int n = 0; int r[kMaxStages]; };
Radices factor(int64_t N) {
    Radices f;
    for (int p : {8, 4, 2, 3, 5, 7})
        while (N % p == 0) { f.r[f.n++] = p; N /= p; }
    return f;
}
// exp(-2 pi i t / M) within about 1 ulp: quadrant and octant taken in integers, the rest in long double on [0, pi/4]
double2 host_root(int64_t t, int64_t M) {
    t %= M;
    if (t < 0) t += M;
    const int64_t a4 = 4 * t, q = a4 / M;
    int64_t r = a4 - q * M;   // angle = q pi/2 + (pi/2) r / M
    const bool comp = 2 * r > M;
    if (comp) r = M - r;
    const long double phi = (long double)M_PI / 2 * ((long double)r / (long double)M);
    long double c = cosl(phi), s = sinl(phi);
    if (comp) std::swap(c, s);
    long double ct, st;
    switch (q) {
        case 0: ct = c; st = s; break;
        case 1: ct = -s; st = c; break;
        case 2: ct = -c; st = -s; break;
        default: ct = s; st = -c; break;
    }
    return make_double2((double)ct, (double)-st);
}

// ---- device: two-table roots -----------------------------------------------------------------------------------------------------
struct RootTab {
    const double2 *lo = nullptr, *hi = nullptr;
    int64_t M = 1;
};
__device__ inline double2 root_of(const RootTab &t, uint64_t r) {
    r %= (uint64_t)t.M;
    const double2 h = t.hi[r / kRootB], l = t.lo[r % kRootB];
    return r < (uint64_t)kRootB ? l : cmul(h, l);
}
// exp(-i pi k^2 / n) = omega_{2n}^(k^2 mod 2n); k < 2^26 keeps k^2 exact in 64 bits
__device__ inline double2 chirp_of(const RootTab &t, int64_t k) { return root_of(t, (uint64_t)k * (uint64_t)k % (uint64_t)t.M); }

struct HostRootTab {
    DevBuf lo, hi;
    RootTab tab;
    int32_t make(int64_t M, hipStream_t s) {
        const int64_t nlo = std::min<int64_t>(M, kRootB), nhi = ceil_div(M, kRootB);
        std::vector<double2> l((size_t)nlo), h((size_t)nhi);
        for (int64_t i = 0; i < nlo; ++i) l[(size_t)i] = host_root(i, M);
        for (int64_t i = 0; i < nhi; ++i) h[(size_t)i] = host_root(i * kRootB, M);
        LPVS_TRY(lo.alloc(sizeof(double2) * (size_t)nlo));
        LPVS_TRY(hi.alloc(sizeof(double2) * (size_t)nhi));
        LPVS_TRY(copy_to_device(lo.p, l.data(), sizeof(double2) * (size_t)nlo, s));
        LPVS_TRY(copy_to_device(hi.p, h.data(), sizeof(double2) * (size_t)nhi, s));
        tab.lo = lo.as<double2>(); tab.hi = hi.as<double2>(); tab.M = M;
        return LPVS_OK;
    }
};
struct HostTwiddles {   // omega_N^t, t < N (N <= 8192): the Stockham stages' twiddles and the small DFTs' roots
    DevBuf buf;
    int32_t make(int64_t N, hipStream_t s) {
        std::vector<double2> w((size_t)N);
        for (int64_t i = 0; i < N; ++i) w[(size_t)i] = host_root(i, N);
        LPVS_TRY(buf.alloc(sizeof(double2) * (size_t)N));
        return copy_to_device(buf.p, w.data(), sizeof(double2) * (size_t)N, s);
    }
};

// ---- epilogue (shared by the LDS kernel and the global-power kernel) ------------------------------------------------------------
template <class T> struct Epi {
    int kind = LPVS_STFT_POWER;
    int64_t nfft = 0, nbins = 0;
    double m1 = 0, m2 = 0;            // 1 / r, 2 / r with r = fs * sum(win.^2)
    const float *W = nullptr;         // band i's weights of bins [blo[i], bhi[i]) at W[woff[i] ...], contiguous
    const int64_t *blo = nullptr, *bhi = nullptr, *woff = nullptr;   // bins [blo[i], bhi[i]) hold band i's non-zero weights
    int nmels = 0;
    const float *D = nullptr;         // nmfcc x nmels, column-major
    int nmfcc = 0;
    T *out = nullptr;                 // rows x frames, column-major
    int64_t nframes = 0;              // frames of the whole call (global frame indices)
    double *wslab = nullptr;          // LPVS_STFT_WELCH: gridDim.x slabs of nbins partial sums
};

__device__ inline double row_scale(int64_t k, int64_t nbins, int64_t nfft, double m1, double m2) {
    if (k == 0) return m1;
    if (k == nbins - 1) return (nfft & 1) ? m2 : m1;
    return m2;
}

// one mel band of one frame: the reference's Float32 weights times Float64 power, summed over the band's bins in ascending order
template <class P>
__device__ inline double mel_band(const float *w, int64_t lo, int64_t hi, const P *pw) {
    double acc = 0.0;
    for (int64_t k = lo; k < hi; ++k) acc = acc + (double)w[k - lo] * (double)pw[k];
    return acc;
}
template <class P>
__device__ inline double dct_coef(const float *D, int nmfcc, int nmels, int j, const P *mel) {
    double acc = 0.0;
    for (int i = 0; i < nmels; ++i) acc = acc + (double)D[j + (int64_t)i * nmfcc] * (double)mel[i];
    return acc;
}
// 2-norm with max-abs scaling: 0 for a zero column (the caller's 0/0 = NaN follows), NaN for a NaN column
__device__ inline double col_norm(const double *c, int n) {
    double amax = 0.0;
    bool nan = false;
    for (int j = 0; j < n; ++j) { const double a = fabs(c[j]); nan |= a != a; amax = a > amax ? a : amax; }
    if (nan) return __builtin_nan("");
    if (amax == 0.0 || isinf(amax)) return amax;
    double ss = 0.0;
    for (int j = 0; j < n; ++j) { const double u = c[j] / amax; ss = ss + u * u; }
    return amax * sqrt(ss);
}

// ---- the LDS FFT ---------------------------------------------------------------------------------------------------------------------
template <class T> struct FftJob {
    int N = 0, nst = 0, rad[kMaxStages] = {};
    const double2 *tw = nullptr;      // omega_N^t
    int B = 1;                        // sequences per workgroup
    int64_t blk0 = 0;                 // first workgroup of this launch (launches are cut at kMaxFftBlocks workgroups)
    int64_t nseq = 0, nsub = 1;       // sequences of this launch, sequences per frame pair
    // input
    int in_mode = IN_SIGNAL;
    const T *s = nullptr, *win = nullptr;
    int64_t n = 0, hop = 0, frame0 = 0, nframes = 0;   // frame length, hop, first frame pair's frame, frames of the call
    const int32_t *fbad = nullptr;    // four-step / fallback: frame_bad_kernel's flags (a flagged frame loads as zeros) ...
    const int32_t *fexp = nullptr;    // ... and max-abs exponents (the quieter frame of a pair is equalised to its partner)
    int chirp_in = 0;                 // Bluestein: x_t * chirp_t for t < nfft (the frame's logical length), 0 above
    int64_t blue_n = 0;
    RootTab chirp;
    const double2 *gin = nullptr;
    int64_t in_ps = 0, in_cs = 0, in_es = 0;
    // after the FFT
    int post = POST_NONE;
    RootTab tw4;                      // four-step twiddle omega_{n1 n2}^(c e)
    const double2 *bhat = nullptr;
    int64_t bhat_cs = 0, bhat_es = 1;
    int64_t blue_m = 0;
    // output
    int out_mode = OUT_GLOBAL;
    double2 *gout = nullptr;
    int64_t out_ps = 0, out_cs = 0, out_es = 0;
    Epi<T> epi;
};

template <int R>
__device__ inline void fft_stage(double2 *buf, int N, int B, int Ns, const double2 *tw) {
    constexpr int MB = (kFftMax / R + kThreads - 1) / kThreads;
    const int NR = N / R, G = B * NR, tws = N / (Ns * R);
    double2 w[R];
#pragma unroll
    for (int q = 0; q < R; ++q) w[q] = tw[q * (N / R)];   // omega_R^q
    double2 v[MB][R];
    int dst[MB];
#pragma unroll
    for (int u = 0; u < MB; ++u) {
        const int g = (int)threadIdx.x + u * kThreads;
        dst[u] = -1;
        if (g < G) {
            const int b = g / NR, j = g - b * NR, k = j % Ns;
            const double2 *x = buf + b * N;
            double2 a[R];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = x[j + r * NR];
#pragma unroll
            for (int r = 1; r < R; ++r) a[r] = cmul(a[r], tw[r * k * tws]);
#pragma unroll
            for (int q = 0; q < R; ++q) {   // direct DFT of length R, exact roots
                double2 acc = a[0];
#pragma unroll
                for (int r = 1; r < R; ++r) {
                    const double2 p = cmul(a[r], w[(q * r) % R]);
                    acc.x = acc.x + p.x; acc.y = acc.y + p.y;
                }
                v[u][q] = acc;
            }
            dst[u] = b * N + (j / Ns) * Ns * R + k;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MB; ++u)
        if (dst[u] >= 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) buf[dst[u] + r * Ns] = v[u][r];
        }
    __syncthreads();
}

template <class T> __device__ inline void run_fft(double2 *buf, const FftJob<T> &J) {
    int Ns = 1;
    for (int st = 0; st < J.nst; ++st) {
        const int R = J.rad[st];
        switch (R) {
            case 8: fft_stage<8>(buf, J.N, J.B, Ns, J.tw); break;
            case 4: fft_stage<4>(buf, J.N, J.B, Ns, J.tw); break;
            case 2: fft_stage<2>(buf, J.N, J.B, Ns, J.tw); break;
            case 3: fft_stage<3>(buf, J.N, J.B, Ns, J.tw); break;
            case 5: fft_stage<5>(buf, J.N, J.B, Ns, J.tw); break;
            default: fft_stage<7>(buf, J.N, J.B, Ns, J.tw); break;
        }
        Ns *= R;
    }
}

// frame flags: a non-finite windowed sample (the frame loads as zeros, its power is NaN), or every windowed sample zero (its power is
// exactly 0: the shared FFT would give it its partner's rounding noise)
enum : int { FRAME_OK = 0, FRAME_NONFINITE = 1, FRAME_ZERO = 2 };
// The rounding error of the shared FFT follows the pair's combined size.  So the quieter frame of a pair is scaled up by 2^s, s the
// difference of the two frames' max-abs exponents, and its power is scaled back by 2^-2s after the split.  Both scales are exact, so
// each frame's error follows its own size and the result does not depend on the partner.
__host__ __device__ inline int pair_shift(int flag, int e, int flag_partner, int e_partner) {
    return (flag == FRAME_OK && flag_partner == FRAME_OK && e_partner > e) ? e_partner - e : 0;
}
__device__ inline int max_exponent(double m) { int e = 0; (void)frexp(m, &e); return e; }
// one bin's power of one frame from its split parts: NaN for a non-finite frame, 0 for an all-zero one, else scaled back by 2^-2s
__device__ inline double frame_power(int flag, int s, double re, double im, double sc) {
    if (flag == FRAME_NONFINITE) return __builtin_nan("");
    if (flag == FRAME_ZERO) return 0.0;
    return ldexp((re * re + im * im) * sc, -2 * s);
}

// element t of frame pair p as one complex value (frame 2p real, 2p+1 imaginary), windowed, zero past the frame; with the flags of
// frame_bad_kernel also zeroed where flagged and equalised (pair_shift)
template <class T> __device__ inline double2 signal_value(const FftJob<T> &J, int64_t p, int64_t t) {
    if (t >= J.n) return make_double2(0.0, 0.0);
    const int64_t fa = J.frame0 + 2 * p, fb = fa + 1;
    const bool hb = fb < J.nframes;
    const double w = J.win ? (double)J.win[t] : 1.0;
    double a = (double)J.s[fa * J.hop + t] * w;
    double b = hb ? (double)J.s[fb * J.hop + t] * w : 0.0;
    if (J.fbad) {
        const int la = J.fbad[fa], lb = hb ? J.fbad[fb] : FRAME_ZERO;
        a = la != FRAME_OK ? 0.0 : ldexp(a, pair_shift(la, J.fexp[fa], lb, hb ? J.fexp[fb] : 0));
        b = lb != FRAME_OK ? 0.0 : ldexp(b, pair_shift(lb, J.fexp[fb], la, J.fexp[fa]));
    }
    return make_double2(a, b);
}

// one workgroup's batch `blk` of J.B sequences: load, FFT, what follows it, output or epilogue.  WELCH: the power columns of the batch
// are added, in ascending frame order, to the per-bin sums wacc (taken as zero when `first`)
template <class T, bool WELCH>
__device__ __forceinline__ void stft_batch(const FftJob<T> &J, int64_t blk, double2 *buf, int *bad, int *shift, double *red, double *wacc, bool first) {
    const int N = J.N, tid = (int)threadIdx.x;
    const int64_t q0 = blk * J.B;
    const int nb = (int)min<int64_t>(J.B, J.nseq - q0);
    // each sequence is one whole frame pair and no frame_bad_kernel pass ran: flag and equalise its frames here
    const bool local = J.in_mode == IN_SIGNAL && J.nsub == 1 && !J.fbad;
    for (int i = tid; i < 2 * kMaxPairs; i += kThreads) { bad[i] = FRAME_OK; shift[i] = 0; }
    __syncthreads();
    // ---- load (local: the windowed samples alone; the flags, the equalisation and the chirp follow once the pair is known)
    for (int i = tid; i < nb * N; i += kThreads) {
        const int b = i / N, e = i - b * N;
        const int64_t q = q0 + b, p = q / J.nsub, c = q - p * J.nsub;
        double2 v;
        if (J.in_mode == IN_SIGNAL) {
            const int64_t t = (int64_t)e * J.nsub + c;
            v = signal_value(J, p, t);
            // flag on the windowed samples themselves: the chirp product mixes the two frames' parts
            if (local) {   // a plain store of 1: the same value from every writer
                if (!isfinite(v.x)) bad[2 * b] = FRAME_NONFINITE;
                if (!isfinite(v.y)) bad[2 * b + 1] = FRAME_NONFINITE;
            } else if (J.chirp_in)
                v = t < J.blue_n ? cmul(v, chirp_of(J.chirp, t)) : make_double2(0.0, 0.0);
        } else
            v = J.gin[p * J.in_ps + c * J.in_cs + (int64_t)e * J.in_es];
        buf[i] = v;
    }
    for (int i = nb * N + tid; i < J.B * N; i += kThreads) buf[i] = make_double2(0.0, 0.0);
    __syncthreads();
    if (local) {
        // the two frames' max |sample| per pair: G threads per pair (a power of two), a butterfly within the wave, then across waves
        int G = 1;
        while (2 * G * J.B <= kThreads) G *= 2;
        const int b = tid / G, l = tid - b * G;
        double ma = 0.0, mb = 0.0;
        if (b < nb)
            for (int e = l; e < N; e += G) { const double2 v = buf[b * N + e]; ma = fmax(ma, fabs(v.x)); mb = fmax(mb, fabs(v.y)); }
        for (int o = 1; o < G && o < 64; o *= 2) { ma = fmax(ma, __shfl_xor(ma, o)); mb = fmax(mb, __shfl_xor(mb, o)); }
        if (G > 64) {   // a pair spans G / 64 waves
            const int w = tid / 64;
            if ((tid & 63) == 0) { red[2 * w] = ma; red[2 * w + 1] = mb; }
            __syncthreads();
            if (l == 0)
                for (int u = 1; u < G / 64; ++u) { ma = fmax(ma, red[2 * (w + u)]); mb = fmax(mb, red[2 * (w + u) + 1]); }
        }
        if (l == 0 && b < nb) {
            const int fa = bad[2 * b] != FRAME_OK ? bad[2 * b] : (ma == 0.0 ? FRAME_ZERO : FRAME_OK);
            const int fb = bad[2 * b + 1] != FRAME_OK ? bad[2 * b + 1] : (mb == 0.0 ? FRAME_ZERO : FRAME_OK);
            const int ea = max_exponent(ma), eb = max_exponent(mb);
            bad[2 * b] = fa; bad[2 * b + 1] = fb;
            shift[2 * b] = pair_shift(fa, ea, fb, eb); shift[2 * b + 1] = pair_shift(fb, eb, fa, ea);
        }
        __syncthreads();
        // a flagged frame loads as zeros (a non-finite sample would spread into its partner), the quieter frame is scaled, then the chirp
        for (int i = tid; i < nb * N; i += kThreads) {
            const int b = i / N, e = i - b * N;
            double2 x = buf[i];
            x.x = bad[2 * b] != FRAME_OK ? 0.0 : ldexp(x.x, shift[2 * b]);
            x.y = bad[2 * b + 1] != FRAME_OK ? 0.0 : ldexp(x.y, shift[2 * b + 1]);
            if (J.chirp_in) x = e < J.blue_n ? cmul(x, chirp_of(J.chirp, e)) : make_double2(0.0, 0.0);
            buf[i] = x;
        }
        __syncthreads();
    }
    run_fft(buf, J);
    // ---- after the FFT (element-wise: every thread touches only its own elements until the barrier)
    if (J.post != POST_NONE) {
        for (int i = tid; i < nb * N; i += kThreads) {
            const int b = i / N, e = i - b * N;
            const int64_t q = q0 + b, c = q - (q / J.nsub) * J.nsub;
            if (J.post == POST_TWIDDLE) buf[i] = cmul(buf[i], root_of(J.tw4, (uint64_t)c * (uint64_t)e));
            else buf[i] = conjd(cmul(buf[i], J.bhat[c * J.bhat_cs + (int64_t)e * J.bhat_es]));
        }
        __syncthreads();
        if (J.post == POST_BLUESTEIN_LDS) {   // inverse by conj-FFT-conj, then the chirp: X_k = chirp_k * ifft(...)_k, k < nfft
            run_fft(buf, J);
            for (int i = tid; i < nb * N; i += kThreads) {
                const int b = i / N, e = i - b * N;
                (void)b;
                if (e < J.blue_n) {
                    double2 z = conjd(buf[i]);
                    z.x = z.x / (double)N; z.y = z.y / (double)N;
                    buf[i] = cmul(z, chirp_of(J.chirp, e));
                }
            }
            __syncthreads();
        }
    }
    if (J.out_mode == OUT_GLOBAL) {
        for (int i = tid; i < nb * N; i += kThreads) {
            const int b = i / N, e = i - b * N;
            const int64_t q = q0 + b, p = q / J.nsub, c = q - p * J.nsub;
            J.gout[p * J.out_ps + c * J.out_cs + (int64_t)e * J.out_es] = buf[i];
        }
        return;
    }
    // ---- split, power (sequence b = frame pair q0 + b; its logical length is nfft)
    const Epi<T> &E = J.epi;
    const int64_t nf = E.nfft, nbins = E.nbins;
    const int items = nb * (int)nbins;
    constexpr int kPer = kSplitPer;
    double pa[kPer], pb[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int it = tid + u * kThreads;
        if (it < items) {
            const int b = it / (int)nbins, k = it - b * (int)nbins;
            const double2 zk = buf[b * N + k], zm = buf[b * N + (k == 0 ? 0 : (int)(nf - k))];
            const double ar = (zk.x + zm.x) * 0.5, ai = (zk.y - zm.y) * 0.5;
            const double br = (zk.y + zm.y) * 0.5, bi = (zm.x - zk.x) * 0.5;
            const double sc = row_scale(k, nbins, nf, E.m1, E.m2);
            pa[u] = frame_power(bad[2 * b], shift[2 * b], ar, ai, sc);
            pb[u] = frame_power(bad[2 * b + 1], shift[2 * b + 1], br, bi, sc);
        }
    }
    __syncthreads();   // every Z read before the power overwrites the buffer
    double *pw = reinterpret_cast<double *>(buf);   // frame f (0 .. 2nb) of this workgroup at pw[f * nbins]
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int it = tid + u * kThreads;
        if (it < items) {
            const int b = it / (int)nbins, k = it - b * (int)nbins;
            const int64_t fa = J.frame0 + 2 * (q0 + b), fb = fa + 1;
            if (E.kind == LPVS_STFT_POWER) {
                E.out[fa * nbins + k] = (T)pa[u];
                if (fb < E.nframes) E.out[fb * nbins + k] = (T)pb[u];
            } else {
                pw[(2 * b) * nbins + k] = pa[u];
                pw[(2 * b + 1) * nbins + k] = pb[u];
                if (!isfinite(pa[u])) bad[2 * b] = FRAME_NONFINITE;        // a plain store: the same value from every writer
                if (!isfinite(pb[u])) bad[2 * b + 1] = FRAME_NONFINITE;
            }
        }
    }
    if (E.kind == LPVS_STFT_POWER) return;
    __syncthreads();
    const int nfr = 2 * nb;
    if constexpr (WELCH) {
        // frames beyond the call's last one (the partner of an odd count's last frame) are skipped; an all-zero frame adds exact zeros
        const int nadd = (int)min<int64_t>((int64_t)nfr, E.nframes - (J.frame0 + 2 * q0));
        for (int k = tid; k < (int)nbins; k += kThreads) {
            double a = first ? 0.0 : wacc[k];
            for (int f = 0; f < nadd; ++f) a = a + pw[(int64_t)f * nbins + k];
            wacc[k] = a;
        }
        return;
    }
    double *mel = pw + (int64_t)nfr * nbins;
    for (int it = tid; it < nfr * E.nmels; it += kThreads) {
        const int f = it / E.nmels, i = it - f * E.nmels;
        const int64_t g = J.frame0 + 2 * q0 + f;
        if (g >= E.nframes) continue;
        const double v = bad[f] == FRAME_NONFINITE ? __builtin_nan("") : mel_band(E.W + E.woff[i], E.blo[i], E.bhi[i], pw + (int64_t)f * nbins);
        if (E.kind == LPVS_STFT_MEL) E.out[g * E.nmels + i] = (T)v;
        else mel[it] = v;
    }
    if (E.kind == LPVS_STFT_MEL) return;
    __syncthreads();
    double *cc = mel + (int64_t)nfr * E.nmels;
    for (int it = tid; it < nfr * E.nmfcc; it += kThreads) {
        const int f = it / E.nmfcc, j = it - f * E.nmfcc;
        cc[it] = dct_coef(E.D, E.nmfcc, E.nmels, j, mel + (int64_t)f * E.nmels);
    }
    __syncthreads();
    for (int f = tid; f < nfr; f += kThreads) {
        const int64_t g = J.frame0 + 2 * q0 + f;
        if (g >= E.nframes) continue;
        const double *c = cc + (int64_t)f * E.nmfcc;
        const double nrm = col_norm(c, E.nmfcc);
        for (int j = 0; j < E.nmfcc; ++j) E.out[g * E.nmfcc + j] = (T)(c[j] / nrm);
    }
}

template <class T>
__global__ void __launch_bounds__(kThreads) stft_fft_kernel(FftJob<T> J) {
    __shared__ double2 buf[kFftMax];
    __shared__ int bad[2 * kMaxPairs];   // frame flags (FRAME_*; a non-finite power value counts as FRAME_NONFINITE)
    __shared__ int shift[2 * kMaxPairs];  // pair_shift of each frame
    __shared__ double red[2 * (kThreads / 64)];
    stft_batch<T, false>(J, J.blk0 + (int64_t)blockIdx.x, buf, bad, shift, red, nullptr, true);
}

// LPVS_STFT_WELCH on the LDS paths: launch r gives batch r gridDim.x + g to workgroup g, which adds the batch's power columns to slab g
// (its own: read and written by this workgroup alone, launch after launch in stream order; the first launch starts from zero)
template <class T>
__global__ void __launch_bounds__(kThreads) stft_welch_kernel(FftJob<T> J) {
    __shared__ double2 buf[kFftMax];
    __shared__ int bad[2 * kMaxPairs];
    __shared__ int shift[2 * kMaxPairs];
    __shared__ double red[2 * (kThreads / 64)];
    stft_batch<T, true>(J, J.blk0 + (int64_t)blockIdx.x, buf, bad, shift, red, J.epi.wslab + (int64_t)blockIdx.x * J.epi.nbins, J.blk0 == 0);
}

// two levels of the pairwise tree over S slabs, in place: slab i <- (slab i + slab i+st) + (slab i+2st + slab i+3st), i = 0, 4 st, ...
__global__ void __launch_bounds__(kEpiThreads) welch_tree_kernel(double *slab, int64_t S, int64_t nbins, int64_t st, int64_t groups) {
    const int64_t idx = (int64_t)blockIdx.x * kEpiThreads + threadIdx.x;
    if (idx >= groups * nbins) return;
    const int64_t g = idx / nbins, k = idx - g * nbins, i = g * 4 * st;
    double v = slab[i * nbins + k];
    if (i + st < S) v = v + slab[(i + st) * nbins + k];
    if (i + 2 * st < S) {
        double w = slab[(i + 2 * st) * nbins + k];
        if (i + 3 * st < S) w = w + slab[(i + 3 * st) * nbins + k];
        v = v + w;
    }
    slab[i * nbins + k] = v;
}
// the mean; two-sided: bins k and nfft - k both get the undoubled value (half the one-sided one, exact)
template <class T>
__global__ void __launch_bounds__(kEpiThreads) welch_finish_kernel(const double *sum, int64_t nbins, int64_t nfft, double frames, int twosided, T *out) {
    const int64_t k = (int64_t)blockIdx.x * kEpiThreads + threadIdx.x;
    if (k >= nbins) return;
    const double v = sum[k] / frames;
    if (!twosided) { out[k] = (T)v; return; }
    const bool edge = k == 0 || ((nfft & 1) == 0 && k == nbins - 1);
    const T h = (T)(edge ? v : 0.5 * v);
    out[k] = h;
    if (!edge) out[nfft - k] = h;
}

constexpr int64_t kMaxFrameBlocks = 65536;   // per-frame kernels stride over the frames beyond this many workgroups
inline unsigned frame_blocks(int64_t count) { return (unsigned)std::min<int64_t>(std::max<int64_t>(count, 1), kMaxFrameBlocks); }

// ---- four-step / Bluestein tail: split + power of a global Z (a workgroup per frame pair, striding over the pairs) ----------------
// bin k of the two frames of one pair from its spectrum z (blue: the inverse FFT by conj-FFT-conj is finished here, then the chirp)
__device__ inline void pair_power(const double2 *z, int64_t k, int64_t nfft, int64_t nbins, double m1, double m2, int blue, const RootTab &chirp,
                                  int64_t m, int la, int sa, int lb, int sb, double &pa, double &pb) {
    const int64_t km = k == 0 ? 0 : nfft - k;
    double2 zk = z[k], zm = z[km];
    if (blue) {
        zk = conjd(zk); zk.x = zk.x / (double)m; zk.y = zk.y / (double)m; zk = cmul(zk, chirp_of(chirp, k));
        zm = conjd(zm); zm.x = zm.x / (double)m; zm.y = zm.y / (double)m; zm = cmul(zm, chirp_of(chirp, km));
    }
    const double ar = (zk.x + zm.x) * 0.5, ai = (zk.y - zm.y) * 0.5;
    const double br = (zk.y + zm.y) * 0.5, bi = (zm.x - zk.x) * 0.5;
    const double sc = row_scale(k, nbins, nfft, m1, m2);
    pa = frame_power(la, sa, ar, ai, sc);
    pb = frame_power(lb, sb, br, bi, sc);
}
template <class T>
__global__ void __launch_bounds__(kEpiThreads) split_power_kernel(const double2 *Z, int64_t zps, int64_t nfft, int64_t nbins, double m1, double m2,
                                                                  int blue, RootTab chirp, int64_t m, int64_t frame0, int64_t nframes,
                                                                  const int32_t *fbad, const int32_t *fexp, T *pw, int64_t pw_frame0, int64_t npairs) {
  for (int64_t p = blockIdx.x; p < npairs; p += gridDim.x) {
    const int64_t fa = frame0 + 2 * p, fb = fa + 1;
    const double2 *z = Z + p * zps;
    const bool hb = fb < nframes;
    const int la = fbad[fa], lb = hb ? fbad[fb] : FRAME_ZERO;
    const int sa = pair_shift(la, fexp[fa], lb, hb ? fexp[fb] : 0), sb = hb ? pair_shift(lb, fexp[fb], la, fexp[fa]) : 0;
    for (int64_t k = threadIdx.x; k < nbins; k += kEpiThreads) {
        double pa, pb;
        pair_power(z, k, nfft, nbins, m1, m2, blue, chirp, m, la, sa, lb, sb, pa, pb);
        pw[(fa - pw_frame0) * nbins + k] = (T)pa;
        if (hb) pw[(fb - pw_frame0) * nbins + k] = (T)pb;
    }
  }
}

// LPVS_STFT_WELCH on the four-step paths: slab j of a chunk = the power of its frame pairs [j P, (j + 1) P), split from Z and added bin
// by bin in ascending frame order (a thread per bin; no power columns are written)
__global__ void __launch_bounds__(kEpiThreads) welch_split_sum_kernel(const double2 *Z, int64_t zps, int64_t nfft, int64_t nbins, double m1, double m2,
                                                                      int blue, RootTab chirp, int64_t m, int64_t frame0, int64_t nframes,
                                                                      const int32_t *fbad, const int32_t *fexp, int64_t npairs, int64_t P, double *slab) {
    const int64_t k = (int64_t)blockIdx.x * kEpiThreads + threadIdx.x, j = blockIdx.y;
    if (k >= nbins) return;
    const int64_t p1 = min((j + 1) * P, npairs);
    double acc = 0.0;
    for (int64_t p = j * P; p < p1; ++p) {
        const int64_t fa = frame0 + 2 * p, fb = fa + 1;
        const bool hb = fb < nframes;
        const int la = fbad[fa], lb = hb ? fbad[fb] : FRAME_ZERO;
        const int sa = pair_shift(la, fexp[fa], lb, hb ? fexp[fb] : 0), sb = hb ? pair_shift(lb, fexp[fb], la, fexp[fa]) : 0;
        double pa, pb;
        pair_power(Z + p * zps, k, nfft, nbins, m1, m2, blue, chirp, m, la, sa, lb, sb, pa, pb);
        acc = acc + pa;
        if (hb) acc = acc + pb;
    }
    slab[j * nbins + k] = acc;
}

// ---- mel / MFCC epilogue from power columns in global memory (a workgroup per frame, striding over the frames) -------------------
template <class P, class T>
__global__ void __launch_bounds__(kEpiThreads) epilogue_kernel(const P *pw, int64_t pw_frame0, Epi<T> E, int64_t frame0, int64_t nfr) {
    extern __shared__ double sh[];   // nmels + nmfcc doubles (MFCC only)
    for (int64_t fl = blockIdx.x; fl < nfr; fl += gridDim.x) {
        const int64_t g = frame0 + fl;
        const P *col = pw + (g - pw_frame0) * E.nbins;
        int bad = 0;
        for (int64_t k = threadIdx.x; k < E.nbins; k += kEpiThreads) bad |= !isfinite((double)col[k]);
        bad = __syncthreads_or(bad);
        for (int i = threadIdx.x; i < E.nmels; i += kEpiThreads) {
            const double v = bad ? __builtin_nan("") : mel_band(E.W + E.woff[i], E.blo[i], E.bhi[i], col);
            if (E.kind == LPVS_STFT_MEL) E.out[g * E.nmels + i] = (T)v;
            else sh[i] = v;
        }
        if (E.kind == LPVS_STFT_MEL) continue;
        __syncthreads();
        double *cc = sh + E.nmels;
        for (int j = threadIdx.x; j < E.nmfcc; j += kEpiThreads) cc[j] = dct_coef(E.D, E.nmfcc, E.nmels, j, sh);
        __syncthreads();
        if (threadIdx.x == 0) {
            const double nrm = col_norm(cc, E.nmfcc);
            for (int j = 0; j < E.nmfcc; ++j) E.out[g * E.nmfcc + j] = (T)(cc[j] / nrm);
        }
        __syncthreads();   // sh is rewritten by the next frame
    }
}

// each frame's flag (FRAME_*) and max-abs exponent, on the windowed samples (a workgroup per frame, striding over the frames; the
// paths whose sequences do not hold whole frame pairs in one workgroup)
template <class T>
__global__ void __launch_bounds__(kEpiThreads) frame_bad_kernel(const T *s, const T *win, int64_t n, int64_t hop, int32_t *fbad, int32_t *fexp,
                                                                int64_t nframes) {
    __shared__ double red[kEpiThreads / 64];
    for (int64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
        int bad = 0;
        double mx = 0.0;
        for (int64_t t = threadIdx.x; t < n; t += kEpiThreads) {
            const double v = (double)s[f * hop + t] * (win ? (double)win[t] : 1.0);   // as signal_value
            bad |= !isfinite(v);
            mx = fmax(mx, fabs(v));
        }
        for (int o = 1; o < 64; o *= 2) mx = fmax(mx, __shfl_xor(mx, o));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = mx;
        bad = __syncthreads_or(bad);
        if (threadIdx.x == 0) {
            for (int w = 1; w < kEpiThreads / 64; ++w) mx = fmax(mx, red[w]);
            fbad[f] = bad ? FRAME_NONFINITE : (mx == 0.0 ? FRAME_ZERO : FRAME_OK);
            fexp[f] = bad ? 0 : max_exponent(mx);
        }
        __syncthreads();   // red is rewritten by the next frame
    }
}

__global__ void bluestein_b_kernel(RootTab chirp, int64_t n, int64_t m, double2 *b) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = j < n ? j : (m - j < n ? m - j : -1);
        b[j] = k < 0 ? make_double2(0.0, 0.0) : conjd(chirp_of(chirp, k));   // conj(chirp_k) = exp(+i pi k^2 / n), k = |j| (mod m)
    }
}

// ---- host plumbing ---------------------------------------------------------------------------------------------------------------
constexpr int kTimingSlots = 11;
thread_local double g_timing[kTimingSlots] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
};
struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};
template <class T> struct Staged {
    DevBuf own;
    const T *p = nullptr;
    int32_t set(const T *src, int64_t count, int dev, hipStream_t s) {
        if (!src || count == 0) { p = src; return LPVS_OK; }
        const int owner = device_of_ptr(src);
        if (owner == dev) { p = src; return LPVS_OK; }
        LPVS_TRY(own.alloc(sizeof(T) * (size_t)count));
        if (owner >= 0) {
            LPVS_HIP(hipMemcpyPeerAsync(own.p, dev, src, owner, sizeof(T) * (size_t)count, s));
            LPVS_HIP(hipStreamSynchronize(s));
        } else
            LPVS_TRY(copy_to_device(own.p, src, sizeof(T) * (size_t)count, s));
        p = own.as<T>();
        return LPVS_OK;
    }
};

// a length <= 2^26 the engine runs: <= 8192 in LDS, else n1 * n2 with both factors <= 8192 and the most balanced such split
struct Plan {
    int64_t len = 0, n1 = 0, n2 = 0;
    bool fits() const { return len > 0; }
};
Plan plan_length(int64_t N) {
    Plan p;
    if (!is_smooth(N) || N > kMaxLen) return p;
    if (N <= kFftMax) { p.len = N; p.n1 = N; p.n2 = 1; return p; }
    int64_t best = 0;
    for (int64_t d = 2; d <= kFftMax; ++d)
        if (N % d == 0 && N / d <= kFftMax && (best == 0 || std::llabs(d * d - N) < std::llabs(best * best - N))) best = d;
    if (best) { p.len = N; p.n1 = best; p.n2 = N / best; }
    return p;
}

// one FFT length on the device: LDS twiddles of its factors and, for the four-step, the twiddle table of n1 n2
struct LengthTables {
    Plan pl;
    HostTwiddles t1, t2;
    HostRootTab t4;
    Radices r1, r2;
    int32_t make(const Plan &p, hipStream_t s) {
        pl = p;
        r1 = factor(p.n1);
        LPVS_TRY(t1.make(p.n1, s));
        if (p.n2 > 1) {
            r2 = factor(p.n2);
            LPVS_TRY(t2.make(p.n2, s));
            LPVS_TRY(t4.make(p.len, s));
        }
        return LPVS_OK;
    }
};

template <class T> void set_fft(FftJob<T> &J, int N, const Radices &r, const double2 *tw, int B, int64_t nseq, int64_t nsub) {
    J.N = N; J.nst = r.n;
    for (int i = 0; i < r.n; ++i) J.rad[i] = r.r[i];
    J.tw = tw; J.B = B; J.nseq = nseq; J.nsub = nsub;
}
constexpr int64_t kMaxFftBlocks = 1 << 20;   // workgroups per launch: keeps blocks x threads far below 2^32
template <class T> int32_t launch_fft(FftJob<T> J, hipStream_t s) {
    const int64_t nblk = J.nseq > 0 ? ceil_div(J.nseq, J.B) : 0;
    for (int64_t b0 = 0; b0 < nblk; b0 += kMaxFftBlocks) {
        J.blk0 = b0;
        stft_fft_kernel<T><<<(unsigned)std::min<int64_t>(kMaxFftBlocks, nblk - b0), kThreads, 0, s>>>(J);
        LPVS_HIP(hipGetLastError());
    }
    return LPVS_OK;
}

// a four-step FFT of npair sequences of length n1 n2 (pair stride ps in `out`).  `J` carries the input mode of pass 1 (the signal or
// global `in`) and, for the Bluestein forward pass, the multiplication by bhat after pass 2.
template <class T> int32_t four_step(FftJob<T> J, const LengthTables &L, int64_t npair, double2 *tmp, double2 *out, int64_t ps, hipStream_t s,
                                     const double2 *bhat) {
    const int64_t n1 = L.pl.n1, n2 = L.pl.n2;
    // pass 1: columns j2 (n2 of them), length n1, times omega^(j2 k1) -> tmp[p][k1][j2]
    FftJob<T> A = J;
    set_fft(A, (int)n1, L.r1, L.t1.buf.as<double2>(), (int)std::max<int64_t>(1, kFftMax / n1), npair * n2, n2);
    if (A.in_mode == IN_GLOBAL) { A.in_cs = 1; A.in_es = n2; }
    A.post = POST_TWIDDLE; A.tw4 = L.t4.tab;
    A.out_mode = OUT_GLOBAL; A.gout = tmp; A.out_ps = ps; A.out_cs = 1; A.out_es = n2;
    LPVS_TRY(launch_fft(A, s));
    // pass 2: rows k1 (n1 of them), length n2 -> out[p][k1 + n1 k2]
    FftJob<T> Bj;
    set_fft(Bj, (int)n2, L.r2, L.t2.buf.as<double2>(), (int)std::max<int64_t>(1, kFftMax / n2), npair * n1, n1);
    Bj.in_mode = IN_GLOBAL; Bj.gin = tmp; Bj.in_ps = ps; Bj.in_cs = n2; Bj.in_es = 1;
    if (bhat) { Bj.post = POST_BLUE_MUL; Bj.bhat = bhat; Bj.bhat_cs = 1; Bj.bhat_es = n1; }
    Bj.out_mode = OUT_GLOBAL; Bj.gout = out; Bj.out_ps = ps; Bj.out_cs = 1; Bj.out_es = n1;
    return launch_fft(Bj, s);
}

int32_t need_device() {
    if (lpvs_device_count() == 0) { set_error("no HIP device visible (the gfx950 path has no CPU fallback)"); return LPVS_EDEVICE; }
    return LPVS_OK;
}

// band i's non-zero weights lie in bins [lo, hi) (each filter's support is contiguous; lo = hi = 0 for an all-zero row)
void band_ranges(const float *W, int64_t nmels, int64_t nbins, std::vector<int64_t> &lo, std::vector<int64_t> &hi) {
    lo.assign((size_t)nmels, -1); hi.assign((size_t)nmels, 0);
    for (int64_t k = 0; k < nbins; ++k) {   // one pass in storage order (W is column-major)
        const float *col = W + k * nmels;
        for (int64_t i = 0; i < nmels; ++i)
            if (col[i] != 0.0f) { if (lo[(size_t)i] < 0) lo[(size_t)i] = k; hi[(size_t)i] = k + 1; }
    }
    for (auto &x : lo) x = x < 0 ? 0 : x;
}

// W / D / band ranges on the device
struct EpiTables {   // W compacted band by band (each band's weights of its bin range, contiguous), the ranges, D
    DevBuf w, d, lo, hi, off;
    int32_t make(const float *W, int64_t nmels, int64_t nbins, const float *D, int64_t nmfcc, int dev, hipStream_t s) {
        std::vector<float> hw;
        const float *Wh = W;
        if (device_of_ptr(W) >= 0) {
            hw.resize((size_t)(nmels * nbins));
            LPVS_TRY(copy_from_device(hw.data(), W, sizeof(float) * hw.size(), s));
            Wh = hw.data();
        }
        std::vector<int64_t> l, h, o((size_t)nmels);
        band_ranges(Wh, nmels, nbins, l, h);
        std::vector<float> wc;
        for (int64_t i = 0; i < nmels; ++i) {
            o[(size_t)i] = (int64_t)wc.size();
            for (int64_t k = l[(size_t)i]; k < h[(size_t)i]; ++k) wc.push_back(Wh[i + k * nmels]);
        }
        if (wc.empty()) wc.push_back(0.0f);
        LPVS_TRY(w.alloc(sizeof(float) * wc.size()));
        LPVS_TRY(copy_to_device(w.p, wc.data(), sizeof(float) * wc.size(), s));
        LPVS_TRY(off.alloc(sizeof(int64_t) * (size_t)nmels));
        LPVS_TRY(copy_to_device(off.p, o.data(), sizeof(int64_t) * (size_t)nmels, s));
        LPVS_TRY(lo.alloc(sizeof(int64_t) * (size_t)nmels));
        LPVS_TRY(hi.alloc(sizeof(int64_t) * (size_t)nmels));
        LPVS_TRY(copy_to_device(lo.p, l.data(), sizeof(int64_t) * (size_t)nmels, s));
        LPVS_TRY(copy_to_device(hi.p, h.data(), sizeof(int64_t) * (size_t)nmels, s));
        if (D && nmfcc > 0) {
            LPVS_TRY(d.alloc(sizeof(float) * (size_t)(nmfcc * nmels)));
            LPVS_TRY(copy_to_device(d.p, D, sizeof(float) * (size_t)(nmfcc * nmels), s));
        }
        (void)dev;
        return LPVS_OK;
    }
};

template <class T>
int32_t stft_impl(int32_t kind, const T *s_in, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const T *window, const float *W,
                  int64_t nmels, const float *D, int64_t nmfcc, int32_t device, T *out, int64_t capacity, int64_t *nframes, int twosided = 0) {
    // ---- arguments (before any device is needed)
    const bool welch = kind == LPVS_STFT_WELCH;   // lpvs_welch only: out holds the mean over the frames, nbins values (nfft two-sided)
    if (kind != LPVS_STFT_POWER && kind != LPVS_STFT_MEL && kind != LPVS_STFT_MFCC && !welch) { set_error("kind must be LPVS_STFT_POWER, _MEL or _MFCC, got %d", kind); return LPVS_EARGUMENT; }
    if (!nframes || (!s_in && L > 0)) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (L < 0 || n < 1) { set_error("need L >= 0 and n >= 1 (L = %lld, n = %lld)", (long long)L, (long long)n); return LPVS_EARGUMENT; }
    if (noverlap < 0 || noverlap >= n) { set_error("noverlap must satisfy 0 <= noverlap < n (noverlap = %lld, n = %lld)", (long long)noverlap, (long long)n); return LPVS_EDOMAIN; }
    if (nfft < n) { set_error("nfft must be >= n (nfft = %lld, n = %lld)", (long long)nfft, (long long)n); return LPVS_EARGUMENT; }
    if (nfft > kMaxLen) { set_error("nfft = %lld exceeds the supported 2^26", (long long)nfft); return LPVS_EUNSUPPORTED; }
    const int64_t nbins = nfft / 2 + 1;
    if ((kind == LPVS_STFT_MEL || kind == LPVS_STFT_MFCC) && (!W || nmels < 1)) { set_error("the mel and MFCC kinds need W and nmels >= 1"); return LPVS_EARGUMENT; }
    if (kind == LPVS_STFT_MFCC && (!D || nmfcc < 1)) { set_error("the MFCC kind needs D and nmfcc >= 1"); return LPVS_EARGUMENT; }
    if (kind == LPVS_STFT_MFCC && nmels + nmfcc > 16384) { set_error("nmels + nmfcc = %lld exceeds 16384", (long long)(nmels + nmfcc)); return LPVS_EUNSUPPORTED; }
    const int64_t hop = n - noverlap;
    const int64_t k = L >= n ? (L - n) / hop + 1 : 0;
    const int64_t rows = welch ? (twosided ? nfft : nbins) : (kind == LPVS_STFT_POWER ? nbins : (kind == LPVS_STFT_MEL ? nmels : nmfcc));
    const int64_t nout = welch ? rows : k * rows;   // output values
    *nframes = k;
    if (welch && k == 0) { set_error("welch_pgram: the signal (L = %lld) is shorter than one frame (n = %lld): the mean over no frame is undefined", (long long)L, (long long)n); return LPVS_EDOMAIN; }
    // Bluestein length: the smallest 7-smooth m >= 2 nfft - 1 the engine runs
    const bool blue = !is_smooth(nfft);
    Plan pl = plan_length(nfft);
    int64_t m = 0;
    if (blue) {
        m = next_smooth(2 * nfft - 1);
        while (m <= kMaxLen && !plan_length(m).fits()) m = next_smooth(m + 1);
        if (m > kMaxLen) { set_error("nfft = %lld is not 7-smooth and its Bluestein length exceeds 2^26", (long long)nfft); return LPVS_EUNSUPPORTED; }
        pl = plan_length(m);
    } else if (!pl.fits()) {
        set_error("nfft = %lld has no split into two factors <= 8192", (long long)nfft);
        return LPVS_EUNSUPPORTED;
    }
    LPVS_TRY(need_device());
    if (!out) return LPVS_OK;   // count only
    if (capacity < nout) { set_error("capacity %lld < %lld outputs (%lld rows x %lld frames)", (long long)capacity, (long long)nout, (long long)rows, (long long)(welch ? 1 : k)); return LPVS_EARGUMENT; }
    if (k == 0) return LPVS_OK;
    LPVS_HIP(hipSetDevice(device));

    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    const hipStream_t s = sh.s;
    Events ev;
    for (auto &x : ev.e) LPVS_HIP(hipEventCreate(&x));
    // ---- window: r = fs * sum(win.^2) (n without a window)
    std::vector<T> hwin;
    double norm2 = (double)n;
    if (window) {
        hwin.resize((size_t)n);
        if (device_of_ptr(window) >= 0) LPVS_TRY(copy_from_device(hwin.data(), window, sizeof(T) * (size_t)n, s));
        else std::memcpy(hwin.data(), window, sizeof(T) * (size_t)n);
        norm2 = 0.0;
        for (int64_t i = 0; i < n; ++i) norm2 = norm2 + (double)hwin[(size_t)i] * (double)hwin[(size_t)i];
    }
    const double r = fs * norm2;

    // ---- memory: outputs plus the minimum scratch must fit, or LPVS_ENOMEM
    const bool dev_out = device_of_ptr(out) == device;
    const int64_t npair_all = (k + 1) / 2;
    const int64_t flen = pl.len;                             // FFT length: nfft, or m for Bluestein
    const bool lds = flen <= kFftMax;
    const size_t per_pair = lds ? 0 : 2 * sizeof(double2) * (size_t)flen;   // tmp + Z
    const size_t power_per_pair = (kind == LPVS_STFT_POWER || welch) ? 0 : 2 * sizeof(double) * (size_t)nbins;
    // LDS paths: frame pairs per workgroup -- the FFT buffer, the power / mel / DCT regions of the epilogue (doubles) and the split's
    // registers must fit; 0 means the epilogue's regions do not fit next to one pair (the fallback through global power columns)
    int64_t lds_b = 0;
    if (lds) {
        const int64_t per_pair_dbl = kind == LPVS_STFT_POWER ? 0 : 2 * (nbins + nmels + (kind == LPVS_STFT_MFCC ? nmfcc : 0));
        lds_b = kFftMax / flen;
        if (per_pair_dbl > 0) lds_b = std::min<int64_t>(lds_b, (2 * kFftMax) / per_pair_dbl);
        lds_b = std::min<int64_t>(std::min<int64_t>(lds_b, kMaxPairs), npair_all);
        while (lds_b > 1 && lds_b * nbins > (int64_t)kSplitPer * kThreads) --lds_b;
        lds_b = std::max<int64_t>(lds_b, 0);
    }
    const bool fallback = lds && lds_b < 1;
    // frame averaging: S slabs of nbins partial sums, at most F frames behind one slab (the header comment has the rule)
    int64_t wS = 0, wF = 0, wcp = 0;
    if (welch && lds) {
        const int64_t nbatch = ceil_div(npair_all, lds_b), bpw = std::max<int64_t>(1, kWelchChain / (2 * lds_b));
        wS = std::max<int64_t>(std::min<int64_t>(nbatch, kWelchSlabs), ceil_div(nbatch, bpw));
        wF = ceil_div(nbatch, wS) * 2 * lds_b - ((nbatch - 1) % wS == 0 ? 2 * lds_b * nbatch - k : 0);
    } else if (welch) {
        wcp = std::max<int64_t>(1, std::min<int64_t>(npair_all, (int64_t)(kScratchBudget / per_pair)));
        for (int64_t p0 = 0; p0 < npair_all; p0 += wcp) {
            const int64_t nfr = std::min<int64_t>(2 * std::min<int64_t>(wcp, npair_all - p0), k - 2 * p0);
            wS += ceil_div(nfr, kWelchChunkFrames);
            wF = std::max<int64_t>(wF, std::min<int64_t>(nfr, kWelchChunkFrames));
        }
    }
    if (wS > ((int64_t)1 << 30)) { set_error("welch_pgram: %lld frames need more than 2^30 slabs", (long long)k); return LPVS_EUNSUPPORTED; }
    int64_t wdepth = 0;
    while (((int64_t)1 << wdepth) < wS) ++wdepth;
    {
        size_t fr = 0, tot = 0;
        LPVS_HIP(hipMemGetInfo(&fr, &tot));
        const size_t avail = fr + pool_cached_bytes(device);
        const size_t need = (dev_out ? 0 : sizeof(T) * (size_t)nout) + sizeof(double) * (size_t)(wS * nbins) + (device_of_ptr(s_in) == device ? 0 : sizeof(T) * (size_t)L) +
                            per_pair + power_per_pair + (blue ? sizeof(double2) * (size_t)m * 3 : 0) +
                            (lds && !fallback ? 0 : 2 * sizeof(int32_t) * (size_t)k) +                    // frame flags, exponents
                            (fallback ? sizeof(double) * (size_t)(k * nbins) + sizeof(double2) * (size_t)(npair_all * flen) : 0);
        if (need > avail) {
            set_error("spectrogram: %lld frames of nfft %lld need %.2f GB of device memory, %.2f GB are free", (long long)k, (long long)nfft,
                      need / 1e9, avail / 1e9);
            return LPVS_ENOMEM;
        }
    }
    LPVS_HIP(hipEventRecord(ev.e[0], s));   // setup: host tables, band ranges, uploads (the stream is idle until e[1])
    Staged<T> ds, dw;
    DevBuf dout, tmp, zbuf, pwbuf, bvec, btmp, bhat, fbad, fexp, wslab;
    DrainOnExit drain(s);
    LPVS_TRY(ds.set(s_in, L, device, s));
    if (window) {
        LPVS_TRY(dw.own.alloc(sizeof(T) * (size_t)n));
        LPVS_TRY(copy_to_device(dw.own.p, hwin.data(), sizeof(T) * (size_t)n, s));
        dw.p = dw.own.template as<T>();
    }
    T *dst = out;
    if (!dev_out) { LPVS_TRY(dout.alloc(sizeof(T) * (size_t)nout)); dst = dout.as<T>(); }
    if (welch) LPVS_TRY(wslab.alloc(sizeof(double) * (size_t)(wS * nbins)));
    EpiTables et;
    if (kind == LPVS_STFT_MEL || kind == LPVS_STFT_MFCC) LPVS_TRY(et.make(W, nmels, nbins, kind == LPVS_STFT_MFCC ? D : nullptr, nmfcc, device, s));
    LengthTables lt;
    LPVS_TRY(lt.make(pl, s));
    HostRootTab chirp;
    if (blue) LPVS_TRY(chirp.make(2 * nfft, s));

    Epi<T> E;
    E.kind = kind; E.nfft = nfft; E.nbins = nbins; E.m1 = 1.0 / r; E.m2 = 2.0 / r;
    E.W = et.w.as<float>(); E.blo = et.lo.as<int64_t>(); E.bhi = et.hi.as<int64_t>(); E.woff = et.off.as<int64_t>(); E.nmels = (int)nmels;
    E.D = et.d.as<float>(); E.nmfcc = (int)nmfcc; E.out = dst; E.nframes = k; E.wslab = wslab.as<double>();

    FftJob<T> J;
    J.in_mode = IN_SIGNAL; J.s = ds.p; J.win = dw.p; J.n = n; J.hop = hop; J.nframes = k;
    if (blue) { J.chirp_in = 1; J.blue_n = nfft; J.chirp = chirp.tab; }
    // the four-step's sequences (and the LDS fallback's split) do not see whole frames: flag the frames and take their max-abs exponents first
    auto flag_frames = [&]() -> int32_t {
        LPVS_TRY(fbad.alloc(sizeof(int32_t) * (size_t)k));
        LPVS_TRY(fexp.alloc(sizeof(int32_t) * (size_t)k));
        frame_bad_kernel<T><<<frame_blocks(k), kEpiThreads, 0, s>>>(ds.p, dw.p, n, hop, fbad.as<int32_t>(), fexp.as<int32_t>(), k);
        LPVS_HIP(hipGetLastError());
        J.fbad = fbad.as<int32_t>(); J.fexp = fexp.as<int32_t>();
        return LPVS_OK;
    };

    LPVS_HIP(hipEventRecord(ev.e[1], s));   // device work from here on
    // Bluestein: bhat = FFT_m(b), b_j = conj(chirp_|j|) for |j| < nfft (indices mod m)
    if (blue) {
        LPVS_TRY(bvec.alloc(sizeof(double2) * (size_t)m));
        LPVS_TRY(bhat.alloc(sizeof(double2) * (size_t)m));
        bluestein_b_kernel<<<(unsigned)std::min<int64_t>(ceil_div(m, 256), 65536), 256, 0, s>>>(chirp.tab, nfft, m, bvec.as<double2>());
        LPVS_HIP(hipGetLastError());
        FftJob<T> Bj;
        Bj.in_mode = IN_GLOBAL; Bj.gin = bvec.as<double2>(); Bj.in_ps = m; Bj.in_es = 1;
        if (lds) {
            set_fft(Bj, (int)m, lt.r1, lt.t1.buf.as<double2>(), 1, 1, 1);
            Bj.out_mode = OUT_GLOBAL; Bj.gout = bhat.as<double2>(); Bj.out_ps = m; Bj.out_es = 1;
            LPVS_TRY(launch_fft(Bj, s));
        } else {
            LPVS_TRY(btmp.alloc(sizeof(double2) * (size_t)m));
            LPVS_TRY(four_step(Bj, lt, 1, btmp.as<double2>(), bhat.as<double2>(), m, s, nullptr));
        }
    }

    int path = 1, B = 1;
    if (lds) {
        const int64_t b = lds_b;
        path = blue ? 3 : 1;
        set_fft(J, (int)flen, lt.r1, lt.t1.buf.as<double2>(), 1, npair_all, 1);
        if (blue) { J.post = POST_BLUESTEIN_LDS; J.bhat = bhat.as<double2>(); J.bhat_cs = 0; J.bhat_es = 1; J.blue_m = m; }
        if (welch) {    // wS workgroups a launch, batch after batch into their slabs
            J.B = (int)b; J.out_mode = OUT_EPI; J.epi = E;
            const int64_t nbatch = ceil_div(npair_all, b);
            for (int64_t b0 = 0; b0 < nbatch; b0 += wS) {
                J.blk0 = b0;
                stft_welch_kernel<T><<<(unsigned)std::min<int64_t>(wS, nbatch - b0), kThreads, 0, s>>>(J);
                LPVS_HIP(hipGetLastError());
            }
            B = (int)b;
        } else if (b >= 1) {   // everything in one launch
            J.B = (int)b; J.out_mode = OUT_EPI; J.epi = E;
            LPVS_TRY(launch_fft(J, s));
            B = (int)b;
        } else {        // the epilogue's LDS regions do not fit next to a frame pair: power columns to global, then the epilogue
            LPVS_TRY(flag_frames());
            LPVS_TRY(pwbuf.alloc(sizeof(double) * (size_t)(k * nbins)));
            J.B = (int)std::max<int64_t>(1, std::min<int64_t>(kFftMax / flen, kMaxPairs));
            J.out_mode = OUT_GLOBAL;
            LPVS_TRY(zbuf.alloc(sizeof(double2) * (size_t)(npair_all * flen)));
            J.gout = zbuf.as<double2>(); J.out_ps = flen; J.out_cs = 0; J.out_es = 1;
            LPVS_TRY(launch_fft(J, s));
            B = 0;
            // Z (already through the Bluestein inverse when blue) -> power
            split_power_kernel<double><<<frame_blocks(npair_all), kEpiThreads, 0, s>>>(zbuf.as<double2>(), flen, nfft, nbins, E.m1, E.m2, 0, RootTab{},
                                                                                      1, 0, k, J.fbad, J.fexp, pwbuf.as<double>(), 0, npair_all);
            LPVS_HIP(hipGetLastError());
            const size_t shb = kind == LPVS_STFT_MFCC ? sizeof(double) * (size_t)(nmels + nmfcc) : 0;
            epilogue_kernel<double, T><<<frame_blocks(k), kEpiThreads, shb, s>>>(pwbuf.as<double>(), 0, E, 0, k);
            LPVS_HIP(hipGetLastError());
        }
    } else {
        path = blue ? 4 : 2;
        LPVS_TRY(flag_frames());
        // chunks of frame pairs: tmp + Z of a chunk within the scratch budget (at least one pair)
        const int64_t cp = std::max<int64_t>(1, std::min<int64_t>(npair_all, (int64_t)(kScratchBudget / per_pair)));
        int64_t wbase = 0;   // slabs written by the chunks so far
        LPVS_TRY(tmp.alloc(sizeof(double2) * (size_t)(cp * flen)));
        LPVS_TRY(zbuf.alloc(sizeof(double2) * (size_t)(cp * flen)));
        if (kind != LPVS_STFT_POWER && !welch) LPVS_TRY(pwbuf.alloc(sizeof(double) * (size_t)(2 * cp * nbins)));
        for (int64_t p0 = 0; p0 < npair_all; p0 += cp) {
            const int64_t np = std::min<int64_t>(cp, npair_all - p0), f0 = 2 * p0;
            FftJob<T> A = J;
            A.frame0 = f0;
            if (blue) {
                // forward FFT_m of the chirped frames (times bhat, conjugated, after pass 2) into Z, then the inverse (a forward FFT of
                // the conjugate) back into Z; the split applies conj / m and the chirp
                LPVS_TRY(four_step(A, lt, np, tmp.as<double2>(), zbuf.as<double2>(), flen, s, bhat.as<double2>()));
                FftJob<T> I;
                I.in_mode = IN_GLOBAL; I.gin = zbuf.as<double2>(); I.in_ps = flen;
                LPVS_TRY(four_step(I, lt, np, tmp.as<double2>(), zbuf.as<double2>(), flen, s, nullptr));
            } else
                LPVS_TRY(four_step(A, lt, np, tmp.as<double2>(), zbuf.as<double2>(), flen, s, nullptr));
            if (welch) {
                const int64_t ns = ceil_div(np, kWelchChunkFrames / 2);
                welch_split_sum_kernel<<<dim3((unsigned)ceil_div(nbins, kEpiThreads), (unsigned)ns), kEpiThreads, 0, s>>>(
                    zbuf.as<double2>(), flen, nfft, nbins, E.m1, E.m2, blue, chirp.tab, m, f0, k, fbad.as<int32_t>(), fexp.as<int32_t>(), np,
                    kWelchChunkFrames / 2, wslab.as<double>() + wbase * nbins);
                LPVS_HIP(hipGetLastError());
                wbase += ns;
            } else if (kind == LPVS_STFT_POWER) {
                split_power_kernel<T><<<frame_blocks(np), kEpiThreads, 0, s>>>(zbuf.as<double2>(), flen, nfft, nbins, E.m1, E.m2, blue, chirp.tab, m,
                                                                               f0, k, fbad.as<int32_t>(), fexp.as<int32_t>(), dst, 0, np);
                LPVS_HIP(hipGetLastError());
            } else {
                split_power_kernel<double><<<frame_blocks(np), kEpiThreads, 0, s>>>(zbuf.as<double2>(), flen, nfft, nbins, E.m1, E.m2, blue,
                                                                                    chirp.tab, m, f0, k, fbad.as<int32_t>(), fexp.as<int32_t>(), pwbuf.as<double>(), f0, np);
                LPVS_HIP(hipGetLastError());
                const int64_t nfr = std::min<int64_t>(2 * np, k - f0);
                const size_t shb = kind == LPVS_STFT_MFCC ? sizeof(double) * (size_t)(nmels + nmfcc) : 0;
                epilogue_kernel<double, T><<<frame_blocks(nfr), kEpiThreads, shb, s>>>(pwbuf.as<double>(), f0, E, f0, nfr);
                LPVS_HIP(hipGetLastError());
            }
        }
    }
    if (welch) {   // the slabs in a fixed pairwise tree (two levels a launch), then the mean
        for (int64_t st = 1; st < wS; st *= 4) {
            const int64_t groups = ceil_div(wS, 4 * st);
            welch_tree_kernel<<<(unsigned)ceil_div(groups * nbins, kEpiThreads), kEpiThreads, 0, s>>>(wslab.as<double>(), wS, nbins, st, groups);
            LPVS_HIP(hipGetLastError());
        }
        welch_finish_kernel<T><<<(unsigned)ceil_div(nbins, kEpiThreads), kEpiThreads, 0, s>>>(wslab.as<double>(), nbins, nfft, (double)k, twosided, dst);
        LPVS_HIP(hipGetLastError());
    }
    LPVS_HIP(hipEventRecord(ev.e[2], s));
    if (!dev_out) LPVS_HIP(hipMemcpyAsync(out, dst, sizeof(T) * (size_t)nout, hipMemcpyDefault, s));
    LPVS_HIP(hipEventRecord(ev.e[3], s));
    LPVS_HIP(hipStreamSynchronize(s));
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) LPVS_HIP(hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]));
    // [0] device work: Bluestein kernel, frame flags, FFTs, epilogue, [1] copy-out, [2] total (setup + [0] + [1]), [3] frames,
    // [4] path (1 LDS, 2 four-step, 3 Bluestein in LDS, 4 Bluestein four-step), [5] FFT length, [6] frame pairs per workgroup (LDS
    // paths; 0 on the LDS fallback through global power columns), [7] rows, [8] setup: host tables, band ranges and uploads
    g_timing[0] = ms[1]; g_timing[1] = ms[2]; g_timing[2] = (double)ms[0] + ms[1] + ms[2]; g_timing[3] = (double)k; g_timing[4] = path;
    g_timing[5] = (double)flen; g_timing[6] = B; g_timing[7] = (double)rows; g_timing[8] = ms[0];
    // [9] LPVS_STFT_WELCH: the longest chain of dependent additions behind one bin, D = F - 1 + ceil(log2 S); [10] its slabs S (0 otherwise)
    g_timing[9] = welch ? (double)(wF - 1 + wdepth) : 0.0; g_timing[10] = (double)wS;
    return LPVS_OK;
}

template <class T>
int32_t mel_project_impl(const T *power, int64_t nbins, int64_t frames, const float *W, int64_t nmels, int32_t device, T *out) {
    if (!power || !W || !out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (nbins < 1 || frames < 0 || nmels < 1) { set_error("need nbins >= 1, frames >= 0, nmels >= 1"); return LPVS_EARGUMENT; }
    LPVS_TRY(need_device());
    if (frames == 0) return LPVS_OK;
    LPVS_HIP(hipSetDevice(device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    const hipStream_t s = sh.s;
    Staged<T> dp;
    DevBuf dout;
    DrainOnExit drain(s);
    LPVS_TRY(dp.set(power, nbins * frames, device, s));
    const bool dev_out = device_of_ptr(out) == device;
    T *dst = out;
    if (!dev_out) { LPVS_TRY(dout.alloc(sizeof(T) * (size_t)(nmels * frames))); dst = dout.as<T>(); }
    EpiTables et;
    LPVS_TRY(et.make(W, nmels, nbins, nullptr, 0, device, s));
    Epi<T> E;
    E.kind = LPVS_STFT_MEL; E.nbins = nbins; E.W = et.w.as<float>(); E.blo = et.lo.as<int64_t>(); E.bhi = et.hi.as<int64_t>(); E.woff = et.off.as<int64_t>();
    E.nmels = (int)nmels; E.out = dst; E.nframes = frames;
    epilogue_kernel<T, T><<<frame_blocks(frames), kEpiThreads, 0, s>>>(dp.p, 0, E, 0, frames);
    LPVS_HIP(hipGetLastError());
    if (!dev_out) LPVS_HIP(hipMemcpyAsync(out, dst, sizeof(T) * (size_t)(nmels * frames), hipMemcpyDefault, s));
    LPVS_HIP(hipStreamSynchronize(s));
    return LPVS_OK;
}

// ---- host: the filterbank and the DCT in the reference's precision (src/mel.jl) ---------------------------------------------------
// Julia's promotion: Int / Float32 arguments keep Float32, Float64 ones widen the grid they enter.  F is the FFT grid's type, G the
// mel grid's type (hz_to_mel / mel_to_hz / mel_frequencies), P their promotion (the weights before the Float32 store).
template <class F> F fft_freq(double fs, int64_t nbins, int64_t k) {   // LinRange(0f0, fs/2f0, nbins)[k]: lerp in double, then rounded
    const F stop = (F)((F)fs / (F)2);
    if (nbins == 1) return (F)0;
    const double t = (double)k / (double)(nbins - 1);
    return (F)((1.0 - t) * (double)(F)0 + t * (double)stop);
}
// log / exp of a Float32 argument: the double result rounded once (correctly rounded but for double-rounding ties)
template <class G> G hz_to_mel_t(G f) {
    const float f_sp = 200.0f / 3;
    const float min_log_hz = 1000.0f, min_log_mel = (min_log_hz - 0.0f) / f_sp, logstep = (float)std::log((double)6.4f) / 27.0f;
    G mel = (f - (G)0.0f) / (G)f_sp;
    if (f >= (G)min_log_hz) mel = (G)min_log_mel + (G)std::log((double)(f / (G)min_log_hz)) / (G)logstep;
    return mel;
}
template <class G> G mel_to_hz_t(G mel) {
    const float f_sp = 200.0f / 3;
    const float min_log_hz = 1000.0f, min_log_mel = (min_log_hz - 0.0f) / f_sp, logstep = (float)std::log((double)6.4f) / 27.0f;
    G f = (G)0.0f + (G)f_sp * mel;
    if (mel >= (G)min_log_mel) f = (G)min_log_hz * (G)std::exp((double)((G)logstep * (mel - (G)min_log_mel)));
    return f;
}
template <class F, class G>
void filterbank(double fs, int64_t nfft, int64_t nmels, double fmin, double fmax, float *W) {
    using P = decltype(F() + G());
    const int64_t nbins = (nfft >> 1) + 1, nm = nmels + 2;
    std::vector<G> mf((size_t)nm);
    const G lo = hz_to_mel_t<G>((G)fmin), hi = hz_to_mel_t<G>((G)fmax);
    for (int64_t j = 0; j < nm; ++j) {   // LinRange(min_mel, max_mel, nm): lerp in double, rounded to G
        const double t = nm == 1 ? 0.0 : (double)j / (double)(nm - 1);
        mf[(size_t)j] = mel_to_hz_t<G>((G)((1.0 - t) * (double)lo + t * (double)hi));
    }
    std::vector<G> enorm((size_t)nmels), d1((size_t)nmels), d2((size_t)nmels);
    for (int64_t i = 0; i < nmels; ++i) {
        enorm[(size_t)i] = (G)2 / (mf[(size_t)i + 2] - mf[(size_t)i]);
        d1[(size_t)i] = mf[(size_t)i + 1] - mf[(size_t)i]; d2[(size_t)i] = mf[(size_t)i + 2] - mf[(size_t)i + 1];
    }
    for (int64_t k = 0; k < nbins; ++k) {   // bins outer: W is written in storage order (column-major)
        const F f = fft_freq<F>(fs, nbins, k);
        for (int64_t i = 0; i < nmels; ++i) {
            const P lower = ((P)f - (P)mf[(size_t)i]) / (P)d1[(size_t)i];
            const P upper = ((P)mf[(size_t)i + 2] - (P)f) / (P)d2[(size_t)i];
            const P mn = lower < upper ? lower : upper;   // min / max propagate NaN in Julia
            P v = (lower != lower || upper != upper) ? (P)NAN : mn;
            v = v != v ? v : (v > (P)0 ? v : (P)0);
            W[i + k * nmels] = (float)(v * (P)enorm[(size_t)i]);
        }
    }
}

}  // namespace
}  // namespace lpvs

using namespace lpvs;

extern "C" {

int32_t lpvs_nextfastfft(int64_t n, int64_t *nfft) {
    if (!nfft) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (n > kMaxLen * 16) { set_error("n = %lld is too large", (long long)n); return LPVS_EARGUMENT; }
    *nfft = next_smooth(n);
    return LPVS_OK;
}

int32_t lpvs_mel_filterbank(double fs, int64_t nfft, int64_t nmels, double fmin, double fmax, int32_t wide, float *W) {
    if (!W) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (nfft < 0 || nmels < 0 || nfft > kMaxLen) { set_error("need 0 <= nfft <= 2^26 and nmels >= 0 (nfft = %lld, nmels = %lld)", (long long)nfft, (long long)nmels); return LPVS_EARGUMENT; }
    const bool wf = wide & 1, wm = (wide & 6) != 0;
    try {
        if (wf && wm) filterbank<double, double>(fs, nfft, nmels, fmin, fmax, W);
        else if (wf) filterbank<double, float>(fs, nfft, nmels, fmin, fmax, W);
        else if (wm) filterbank<float, double>(fs, nfft, nmels, fmin, fmax, W);
        else filterbank<float, float>(fs, nfft, nmels, fmin, fmax, W);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
    return LPVS_OK;
}

int32_t lpvs_dct_matrix(int64_t nfilters, int64_t ninput, float *D) {
    if (!D) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (nfilters < 0 || ninput < 1) { set_error("need nfilters >= 0 and ninput >= 1"); return LPVS_EARGUMENT; }
    // samples = (1f0:2f0:2ninput) * pi / 2ninput in Float32; basis[i, :] = cos.(i * samples); basis *= sqrt(2f0 / ninput)
    const float sc = std::sqrt(2.0f / (float)ninput);
    for (int64_t j = 0; j < ninput; ++j) {
        const float smp = (float)(2 * j + 1) * (float)M_PI / (float)(2 * ninput);
        for (int64_t i = 1; i <= nfilters; ++i) D[(i - 1) + j * nfilters] = std::cos((float)i * smp) * sc;
    }
    return LPVS_OK;
}

int32_t lpvs_stft_f64(int32_t kind, const double *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const double *window,
                      const float *W, int64_t nmels, const float *D, int64_t nmfcc, int32_t device, double *out, int64_t capacity,
                      int64_t *nframes) {
    if (kind == LPVS_STFT_WELCH) { set_error("LPVS_STFT_WELCH is the epilogue of lpvs_welch (lpvs_stft has no frame-averaged output)"); return LPVS_EARGUMENT; }
    try {
        return stft_impl(kind, s, L, n, noverlap, nfft, fs, window, W, nmels, D, nmfcc, device, out, capacity, nframes);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_stft_f32(int32_t kind, const float *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const float *window,
                      const float *W, int64_t nmels, const float *D, int64_t nmfcc, int32_t device, float *out, int64_t capacity,
                      int64_t *nframes) {
    if (kind == LPVS_STFT_WELCH) { set_error("LPVS_STFT_WELCH is the epilogue of lpvs_welch (lpvs_stft has no frame-averaged output)"); return LPVS_EARGUMENT; }
    try {
        return stft_impl(kind, s, L, n, noverlap, nfft, fs, window, W, nmels, D, nmfcc, device, out, capacity, nframes);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_welch_f64(const double *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const double *window, int32_t onesided,
                       int32_t device, double *out, int64_t *nframes) {
    if (!out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    try {
        return stft_impl(LPVS_STFT_WELCH, s, L, n, noverlap, nfft, fs, window, nullptr, 0, nullptr, 0, device, out, onesided ? nfft / 2 + 1 : nfft,
                         nframes, onesided ? 0 : 1);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_welch_f32(const float *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const float *window, int32_t onesided,
                       int32_t device, float *out, int64_t *nframes) {
    if (!out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    try {
        return stft_impl(LPVS_STFT_WELCH, s, L, n, noverlap, nfft, fs, window, nullptr, 0, nullptr, 0, device, out, onesided ? nfft / 2 + 1 : nfft,
                         nframes, onesided ? 0 : 1);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_mel_project_f64(const double *power, int64_t nbins, int64_t frames, const float *W, int64_t nmels, int32_t device, double *out) {
    try { return mel_project_impl(power, nbins, frames, W, nmels, device, out); }
    catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_mel_project_f32(const float *power, int64_t nbins, int64_t frames, const float *W, int64_t nmels, int32_t device, float *out) {
    try { return mel_project_impl(power, nbins, frames, W, nmels, device, out); }
    catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_stft_last_timing(double *out, int32_t n) {
    if (!out || n < 0) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    for (int32_t k = 0; k < n && k < kTimingSlots; ++k) out[k] = g_timing[k];
    return LPVS_OK;
}

}  // extern "C"
