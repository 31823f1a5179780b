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
// A second kernel adds the slabs in a fixed pairwise tree and a third divides by the frame count.
// Which path a call takes, its frame pairs per workgroup, its chunks, its slabs with their sum chain and the memory it needs are decided
// in stft_plan.h (StftPlan: pure host arithmetic, tested without a device); stft_impl below runs one function per phase of that plan.
#include "lpvs_internal.h"
#include "stft_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace lpvs {
namespace {

// (kFftMax, kThreads, kMaxStages, kMaxPairs, kSplitPer, kMaxLen, the scratch budget and the frame average's constants: stft_plan.h)
constexpr int64_t kRootB = 8192;     // two-table roots: r = hi * kRootB + lo
constexpr int kEpiThreads = 256;

enum : int { IN_SIGNAL = 0, IN_GLOBAL = 1 };
enum : int { POST_NONE = 0, POST_TWIDDLE = 1, POST_BLUE_MUL = 2, POST_BLUESTEIN_LDS = 3 };
enum : int { OUT_GLOBAL = 0, OUT_EPI = 1 };

__host__ __device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline double2 conjd(double2 a) { return make_double2(a.x, -a.y); }

// ---- host: roots (7-smooth lengths and their factorisation: stft_plan.h) -------------------------------------------------------------
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

// one FFT length on the device: LDS twiddles of its factors and, for the four-step, the twiddle table of n1 n2
struct LengthTables {
    FftSplit pl;
    HostTwiddles t1, t2;
    HostRootTab t4;
    Radices r1, r2;
    int32_t make(const FftSplit &p, hipStream_t s) {
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
    set_fft(A, (int)n1, L.r1, L.t1.buf.as<double2>(), fft_batch(n1), npair * n2, n2);
    if (A.in_mode == IN_GLOBAL) { A.in_cs = 1; A.in_es = n2; }
    A.post = POST_TWIDDLE; A.tw4 = L.t4.tab;
    A.out_mode = OUT_GLOBAL; A.gout = tmp; A.out_ps = ps; A.out_cs = 1; A.out_es = n2;
    LPVS_TRY(launch_fft(A, s));
    // pass 2: rows k1 (n1 of them), length n2 -> out[p][k1 + n1 k2]
    FftJob<T> Bj;
    set_fft(Bj, (int)n2, L.r2, L.t2.buf.as<double2>(), fft_batch(n2), npair * n1, n1);
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

// ---- one STFT call, phase by phase (every number that is decided: StftPlan) -----------------------------------------------------
// the arguments, before any device is needed (LPVS_STFT_WELCH is lpvs_welch's only: out holds the mean over the frames)
template <class T>
int32_t check_stft_arguments(int32_t kind, const T *s_in, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, const float *W, int64_t nmels,
                             const float *D, int64_t nmfcc, const int64_t *nframes) {
    if (kind != LPVS_STFT_POWER && kind != LPVS_STFT_MEL && kind != LPVS_STFT_MFCC && kind != LPVS_STFT_WELCH) { set_error("kind must be LPVS_STFT_POWER, _MEL or _MFCC, got %d", kind); return LPVS_EARGUMENT; }
    if (!nframes || (!s_in && L > 0)) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (L < 0 || n < 1) { set_error("need L >= 0 and n >= 1 (L = %lld, n = %lld)", (long long)L, (long long)n); return LPVS_EARGUMENT; }
    if (noverlap < 0 || noverlap >= n) { set_error("noverlap must satisfy 0 <= noverlap < n (noverlap = %lld, n = %lld)", (long long)noverlap, (long long)n); return LPVS_EDOMAIN; }
    if (nfft < n) { set_error("nfft must be >= n (nfft = %lld, n = %lld)", (long long)nfft, (long long)n); return LPVS_EARGUMENT; }
    if (nfft > kMaxLen) { set_error("nfft = %lld exceeds the supported 2^26", (long long)nfft); return LPVS_EUNSUPPORTED; }
    if ((kind == LPVS_STFT_MEL || kind == LPVS_STFT_MFCC) && (!W || nmels < 1)) { set_error("the mel and MFCC kinds need W and nmels >= 1"); return LPVS_EARGUMENT; }
    if (kind == LPVS_STFT_MFCC && (!D || nmfcc < 1)) { set_error("the MFCC kind needs D and nmfcc >= 1"); return LPVS_EARGUMENT; }
    if (kind == LPVS_STFT_MFCC && nmels + nmfcc > 16384) { set_error("nmels + nmfcc = %lld exceeds 16384", (long long)(nmels + nmfcc)); return LPVS_EUNSUPPORTED; }
    return LPVS_OK;
}
// what the plan refuses, as a status and a message
int32_t refusal_status(const StftPlan &P) {
    switch (P.refusal) {
        case kStftOk: return LPVS_OK;
        case kStftNfftTooLong: set_error("nfft = %lld exceeds the supported 2^26", (long long)P.nfft); return LPVS_EUNSUPPORTED;
        case kStftNoSplit: set_error("nfft = %lld has no split into two factors <= 8192", (long long)P.nfft); return LPVS_EUNSUPPORTED;
        case kStftBluesteinTooLong: set_error("nfft = %lld is not 7-smooth and its Bluestein length exceeds 2^26", (long long)P.nfft); return LPVS_EUNSUPPORTED;
        case kStftTooManySlabs: set_error("welch_pgram: %lld frames need more than 2^30 slabs", (long long)P.frames); return LPVS_EUNSUPPORTED;
        case kStftWelchNoPair: break;
    }
    set_error("internal: the frame average of nfft = %lld has no room for a frame pair in LDS", (long long)P.nfft);
    return LPVS_EASSERT;
}

// the device buffers of a call, in stft_impl BEFORE its DrainOnExit (they return to the pool once the stream is idle); the tables after it
template <class T> struct StftBuffers {
    Staged<T> ds, dw;
    DevBuf dout, tmp, zbuf, pwbuf, bvec, btmp, bhat, fbad, fexp, wslab;
    T *dst = nullptr;   // the output on the device: the caller's array, or dout
};
struct StftTables {
    EpiTables et;
    LengthTables lt;
    HostRootTab chirp;
};
// how the split undoes Bluestein after the four-step inverse: conj / m and the chirp (spectra through the LDS inverse need neither)
struct Unchirp {
    int blue = 0;
    RootTab chirp;
    int64_t m = 0;
};

// r / fs = sum(win.^2) (n without a window); hwin: the window on the host
template <class T> int32_t window_norm(const T *window, int64_t n, hipStream_t s, std::vector<T> &hwin, double *norm2) {
    *norm2 = (double)n;
    if (!window) return LPVS_OK;
    hwin.resize((size_t)n);
    if (device_of_ptr(window) >= 0) LPVS_TRY(copy_from_device(hwin.data(), window, sizeof(T) * (size_t)n, s));
    else std::memcpy(hwin.data(), window, sizeof(T) * (size_t)n);
    *norm2 = 0.0;
    for (int64_t i = 0; i < n; ++i) *norm2 = *norm2 + (double)hwin[(size_t)i] * (double)hwin[(size_t)i];
    return LPVS_OK;
}

// the slabs must be countable and the outputs plus the minimum scratch must fit, or LPVS_ENOMEM
int32_t admit(const StftPlan &P, size_t elt, bool dev_out, bool dev_signal, int device) {
    LPVS_TRY(refusal_status(P));
    size_t fr = 0, tot = 0;
    LPVS_HIP(hipMemGetInfo(&fr, &tot));
    const size_t avail = fr + pool_cached_bytes(device), need = stft_device_bytes(P, elt, dev_out, dev_signal);
    if (need > avail) {
        set_error("spectrogram: %lld frames of nfft %lld need %.2f GB of device memory, %.2f GB are free", (long long)P.frames, (long long)P.nfft,
                  need / 1e9, avail / 1e9);
        return LPVS_ENOMEM;
    }
    return LPVS_OK;
}

// the signal, the window and the output on the device, the slabs, the epilogue's and the lengths' tables
template <class T>
int32_t stage_inputs(const StftPlan &P, const T *s_in, const std::vector<T> &hwin, const float *W, const float *D, int device, T *out, bool dev_out,
                     hipStream_t s, StftBuffers<T> &b, StftTables &t) {
    LPVS_TRY(b.ds.set(s_in, P.L, device, s));
    if (!hwin.empty()) {
        LPVS_TRY(b.dw.own.alloc(sizeof(T) * (size_t)P.n));
        LPVS_TRY(copy_to_device(b.dw.own.p, hwin.data(), sizeof(T) * (size_t)P.n, s));
        b.dw.p = b.dw.own.template as<T>();
    }
    b.dst = out;
    if (!dev_out) { LPVS_TRY(b.dout.alloc(P.out_bytes(sizeof(T)))); b.dst = b.dout.template as<T>(); }
    if (P.welch) LPVS_TRY(b.wslab.alloc(P.slab_bytes()));
    if (P.kind == LPVS_STFT_MEL || P.kind == LPVS_STFT_MFCC)
        LPVS_TRY(t.et.make(W, P.nmels, P.nbins, P.kind == LPVS_STFT_MFCC ? D : nullptr, P.nmfcc, device, s));
    LPVS_TRY(t.lt.make(P.split, s));
    if (P.blue) LPVS_TRY(t.chirp.make(2 * P.nfft, s));
    return LPVS_OK;
}

// the four-step's sequences (and the LDS fallback's split) do not see whole frames: flag the frames and take their max-abs exponents first
template <class T> int32_t flag_frames(const StftPlan &P, FftJob<T> &J, StftBuffers<T> &b, hipStream_t s) {
    LPVS_TRY(b.fbad.alloc(P.flag_bytes()));
    LPVS_TRY(b.fexp.alloc(P.flag_bytes()));
    frame_bad_kernel<T><<<frame_blocks(P.frames), kEpiThreads, 0, s>>>(b.ds.p, b.dw.p, P.n, P.hop, b.fbad.template as<int32_t>(), b.fexp.template as<int32_t>(), P.frames);
    LPVS_HIP(hipGetLastError());
    J.fbad = b.fbad.template as<int32_t>(); J.fexp = b.fexp.template as<int32_t>();
    return LPVS_OK;
}

// Bluestein: bhat = FFT_m(b), b_j = conj(chirp_|j|) for |j| < nfft (indices mod m)
template <class T> int32_t bluestein_bhat(const StftPlan &P, const StftTables &t, StftBuffers<T> &b, hipStream_t s) {
    const int64_t m = P.m;
    LPVS_TRY(b.bvec.alloc(P.bluestein_bytes()));
    LPVS_TRY(b.bhat.alloc(P.bluestein_bytes()));
    bluestein_b_kernel<<<(unsigned)std::min<int64_t>(ceil_div(m, 256), 65536), 256, 0, s>>>(t.chirp.tab, P.nfft, m, b.bvec.template as<double2>());
    LPVS_HIP(hipGetLastError());
    FftJob<T> Bj;
    Bj.in_mode = IN_GLOBAL; Bj.gin = b.bvec.template as<double2>(); Bj.in_ps = m; Bj.in_es = 1;
    if (P.lds) {
        set_fft(Bj, (int)m, t.lt.r1, t.lt.t1.buf.template as<double2>(), 1, 1, 1);
        Bj.out_mode = OUT_GLOBAL; Bj.gout = b.bhat.template as<double2>(); Bj.out_ps = m; Bj.out_es = 1;
        return launch_fft(Bj, s);
    }
    LPVS_TRY(b.btmp.alloc(P.bluestein_bytes()));
    return four_step(Bj, t.lt, 1, b.btmp.template as<double2>(), b.bhat.template as<double2>(), m, s, nullptr);
}

// np frame pairs' spectra in zbuf, the first of them frame f0's -> power rows of the output, the slabs from *wbase on, or power columns
// and the epilogue
template <class T>
int32_t spectra_to_output(const StftPlan &P, const Epi<T> &E, const StftBuffers<T> &b, const Unchirp &u, int64_t f0, int64_t np, int64_t *wbase, hipStream_t s) {
    const double2 *Z = b.zbuf.template as<double2>();
    const int32_t *fbad = b.fbad.template as<int32_t>(), *fexp = b.fexp.template as<int32_t>();
    const int64_t flen = P.split.len, nfr = std::min<int64_t>(2 * np, P.frames - f0);
    if (P.welch) {
        const int64_t ns = welch_chunk_slabs(nfr);
        welch_split_sum_kernel<<<dim3((unsigned)ceil_div(P.nbins, kEpiThreads), (unsigned)ns), kEpiThreads, 0, s>>>(
            Z, flen, P.nfft, P.nbins, E.m1, E.m2, u.blue, u.chirp, u.m, f0, P.frames, fbad, fexp, np, kWelchChunkPairs,
            b.wslab.template as<double>() + *wbase * P.nbins);
        LPVS_HIP(hipGetLastError());
        *wbase += ns;
    } else if (P.power_columns()) {
        split_power_kernel<double><<<frame_blocks(np), kEpiThreads, 0, s>>>(Z, flen, P.nfft, P.nbins, E.m1, E.m2, u.blue, u.chirp, u.m, f0, P.frames, fbad,
                                                                            fexp, b.pwbuf.template as<double>(), f0, np);
        LPVS_HIP(hipGetLastError());
        const size_t shb = P.kind == LPVS_STFT_MFCC ? sizeof(double) * (size_t)(P.nmels + P.nmfcc) : 0;
        epilogue_kernel<double, T><<<frame_blocks(nfr), kEpiThreads, shb, s>>>(b.pwbuf.template as<double>(), f0, E, f0, nfr);
        LPVS_HIP(hipGetLastError());
    } else {
        split_power_kernel<T><<<frame_blocks(np), kEpiThreads, 0, s>>>(Z, flen, P.nfft, P.nbins, E.m1, E.m2, u.blue, u.chirp, u.m, f0, P.frames, fbad, fexp,
                                                                       b.dst, 0, np);
        LPVS_HIP(hipGetLastError());
    }
    return LPVS_OK;
}

// the LDS paths: everything in one launch; the frame average batch after batch into its slabs; or the fallback
template <class T>
int32_t run_lds(const StftPlan &P, FftJob<T> J, const Epi<T> &E, const StftTables &t, StftBuffers<T> &b, hipStream_t s) {
    const int64_t flen = P.split.len;
    set_fft(J, (int)flen, t.lt.r1, t.lt.t1.buf.template as<double2>(), 1, P.pairs, 1);
    if (P.blue) { J.post = POST_BLUESTEIN_LDS; J.bhat = b.bhat.template as<double2>(); J.bhat_cs = 0; J.bhat_es = 1; J.blue_m = P.m; }
    if (!P.fallback) {
        J.B = (int)P.pairs_per_workgroup; J.out_mode = OUT_EPI; J.epi = E;
        if (!P.welch) return launch_fft(J, s);
        for (int64_t b0 = 0; b0 < P.batches; b0 += P.slabs) {   // the same P.slabs workgroups a launch, each into its own slab
            J.blk0 = b0;
            stft_welch_kernel<T><<<(unsigned)std::min<int64_t>(P.slabs, P.batches - b0), kThreads, 0, s>>>(J);
            LPVS_HIP(hipGetLastError());
        }
        return LPVS_OK;
    }
    // the epilogue's LDS regions do not fit next to a frame pair: spectra (already through the Bluestein inverse) to global, then as a chunk
    LPVS_TRY(flag_frames(P, J, b, s));
    LPVS_TRY(b.pwbuf.alloc(P.fallback_power_bytes()));
    J.B = P.fallback_batch;
    J.out_mode = OUT_GLOBAL;
    LPVS_TRY(b.zbuf.alloc(P.fallback_spectra_bytes()));
    J.gout = b.zbuf.template as<double2>(); J.out_ps = flen; J.out_cs = 0; J.out_es = 1;
    LPVS_TRY(launch_fft(J, s));
    Unchirp none;
    none.m = 1;
    return spectra_to_output(P, E, b, none, 0, P.pairs, nullptr, s);
}

// the four-step paths: chunks of P.chunk_pairs frame pairs through global scratch
template <class T>
int32_t run_four_step(const StftPlan &P, FftJob<T> J, const Epi<T> &E, const StftTables &t, StftBuffers<T> &b, hipStream_t s) {
    const int64_t flen = P.split.len, cp = P.chunk_pairs;
    LPVS_TRY(flag_frames(P, J, b, s));
    LPVS_TRY(b.tmp.alloc((size_t)cp * P.pair_spectrum_bytes()));
    LPVS_TRY(b.zbuf.alloc((size_t)cp * P.pair_spectrum_bytes()));
    if (P.power_columns()) LPVS_TRY(b.pwbuf.alloc((size_t)cp * P.pair_power_bytes()));
    double2 *tmp = b.tmp.template as<double2>(), *Z = b.zbuf.template as<double2>();
    Unchirp u;
    u.blue = P.blue; u.chirp = t.chirp.tab; u.m = P.m;
    int64_t wbase = 0;   // slabs written by the chunks so far
    for (int64_t p0 = 0; p0 < P.pairs; p0 += cp) {
        const int64_t np = std::min<int64_t>(cp, P.pairs - p0);
        FftJob<T> A = J;
        A.frame0 = 2 * p0;
        if (P.blue) {
            // forward FFT_m of the chirped frames (times bhat, conjugated, after pass 2) into Z, then the inverse (a forward FFT of
            // the conjugate) back into Z; the split applies conj / m and the chirp
            LPVS_TRY(four_step(A, t.lt, np, tmp, Z, flen, s, b.bhat.template as<double2>()));
            FftJob<T> I;
            I.in_mode = IN_GLOBAL; I.gin = Z; I.in_ps = flen;
            LPVS_TRY(four_step(I, t.lt, np, tmp, Z, flen, s, nullptr));
        } else
            LPVS_TRY(four_step(A, t.lt, np, tmp, Z, flen, s, nullptr));
        LPVS_TRY(spectra_to_output(P, E, b, u, 2 * p0, np, &wbase, s));
    }
    return LPVS_OK;
}

// the slabs in a fixed pairwise tree (two levels a launch), then the mean
template <class T> int32_t welch_reduce(const StftPlan &P, const StftBuffers<T> &b, hipStream_t s) {
    double *slab = b.wslab.template as<double>();
    for (int64_t st = 1; st < P.slabs; st *= 4) {
        const int64_t groups = ceil_div(P.slabs, 4 * st);
        welch_tree_kernel<<<(unsigned)ceil_div(groups * P.nbins, kEpiThreads), kEpiThreads, 0, s>>>(slab, P.slabs, P.nbins, st, groups);
        LPVS_HIP(hipGetLastError());
    }
    welch_finish_kernel<T><<<(unsigned)ceil_div(P.nbins, kEpiThreads), kEpiThreads, 0, s>>>(slab, P.nbins, P.nfft, (double)P.frames, P.twosided, b.dst);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

// [0] device work: Bluestein kernel, frame flags, FFTs, epilogue, [1] copy-out, [2] total (setup + [0] + [1]), [3] frames,
// [4] path (1 LDS, 2 four-step, 3 Bluestein in LDS, 4 Bluestein four-step), [5] FFT length, [6] frame pairs per workgroup (LDS
// paths; 0 on the LDS fallback through global power columns), [7] rows, [8] setup: host tables, band ranges and uploads,
// [9] LPVS_STFT_WELCH: the longest chain of dependent additions behind one bin (StftPlan::sum_chain), [10] its slabs S (0 otherwise)
int32_t report_timing(const StftPlan &P, const Events<4> &ev) {
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) LPVS_HIP(hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]));
    g_timing[0] = ms[1]; g_timing[1] = ms[2]; g_timing[2] = (double)ms[0] + ms[1] + ms[2]; g_timing[3] = (double)P.frames; g_timing[4] = P.path;
    g_timing[5] = (double)P.split.len; g_timing[6] = P.lds ? (double)P.pairs_per_workgroup : 1.0; g_timing[7] = (double)P.rows; g_timing[8] = ms[0];
    g_timing[9] = (double)P.sum_chain; g_timing[10] = (double)P.slabs;
    return LPVS_OK;
}

template <class T>
int32_t stft_impl(int32_t kind, const T *s_in, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const T *window, const float *W,
                  int64_t nmels, const float *D, int64_t nmfcc, int32_t device, T *out, int64_t capacity, int64_t *nframes, int twosided = 0) {
    LPVS_TRY(check_stft_arguments(kind, s_in, L, n, noverlap, nfft, W, nmels, D, nmfcc, nframes));
    const StftPlan P = stft_plan(kind, L, n, noverlap, nfft, nmels, nmfcc, twosided != 0);
    *nframes = P.frames;
    if (P.welch && P.frames == 0) { set_error("welch_pgram: the signal (L = %lld) is shorter than one frame (n = %lld): the mean over no frame is undefined", (long long)L, (long long)n); return LPVS_EDOMAIN; }
    if (P.refusal != kStftTooManySlabs) LPVS_TRY(refusal_status(P));   // (the slabs are refused where the memory is: admit)
    LPVS_TRY(need_device());
    if (!out) return LPVS_OK;   // count only
    if (capacity < P.nout) { set_error("capacity %lld < %lld outputs (%lld rows x %lld frames)", (long long)capacity, (long long)P.nout, (long long)P.rows, (long long)(P.welch ? 1 : P.frames)); return LPVS_EARGUMENT; }
    if (P.frames == 0) return LPVS_OK;
    LPVS_HIP(hipSetDevice(device));

    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    const hipStream_t s = sh.s;
    Events<4> ev;
    for (auto &x : ev.e) LPVS_HIP(hipEventCreate(&x));
    std::vector<T> hwin;
    double norm2 = 0;
    LPVS_TRY(window_norm(window, n, s, hwin, &norm2));
    const double r = fs * norm2;
    const bool dev_out = device_of_ptr(out) == device;
    LPVS_TRY(admit(P, sizeof(T), dev_out, device_of_ptr(s_in) == device, device));

    LPVS_HIP(hipEventRecord(ev.e[0], s));   // setup: host tables, band ranges, uploads (the stream is idle until e[1])
    StftBuffers<T> b;
    DrainOnExit drain(s);
    StftTables t;
    LPVS_TRY(stage_inputs(P, s_in, hwin, W, D, device, out, dev_out, s, b, t));
    Epi<T> E;
    E.kind = kind; E.nfft = nfft; E.nbins = P.nbins; E.m1 = 1.0 / r; E.m2 = 2.0 / r;
    E.W = t.et.w.as<float>(); E.blo = t.et.lo.as<int64_t>(); E.bhi = t.et.hi.as<int64_t>(); E.woff = t.et.off.as<int64_t>(); E.nmels = (int)nmels;
    E.D = t.et.d.as<float>(); E.nmfcc = (int)nmfcc; E.out = b.dst; E.nframes = P.frames; E.wslab = b.wslab.template as<double>();
    FftJob<T> J;
    J.in_mode = IN_SIGNAL; J.s = b.ds.p; J.win = b.dw.p; J.n = n; J.hop = P.hop; J.nframes = P.frames;
    if (P.blue) { J.chirp_in = 1; J.blue_n = nfft; J.chirp = t.chirp.tab; }

    // Kernels lie in the code object in the order they are first named.  The flag pass is named here, ahead of the FFT kernels, where it
    // has always lain: with it behind them the same kernels ran the Bluestein four-step path 0.04 ms slower (profiles/stft_plan_ab.txt).
    (void)&flag_frames<T>;
    LPVS_HIP(hipEventRecord(ev.e[1], s));   // device work from here on
    if (P.blue) LPVS_TRY(bluestein_bhat(P, t, b, s));
    LPVS_TRY(P.lds ? run_lds(P, J, E, t, b, s) : run_four_step(P, J, E, t, b, s));
    if (P.welch) LPVS_TRY(welch_reduce(P, b, s));
    LPVS_HIP(hipEventRecord(ev.e[2], s));
    if (!dev_out) LPVS_HIP(hipMemcpyAsync(out, b.dst, P.out_bytes(sizeof(T)), hipMemcpyDefault, s));
    LPVS_HIP(hipEventRecord(ev.e[3], s));
    LPVS_HIP(hipStreamSynchronize(s));
    return report_timing(P, ev);
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
    return copy_timing(out, n, g_timing, kTimingSlots);
}

}  // extern "C"
