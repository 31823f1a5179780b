// autocov.hip -- autocov / autocor of signals sampled at arbitrary times (src/autocov.jl) on gfx950.
//
// Every sample pair (i, j >= 0, i+j < N) of every segment is a candidate; the pairs with tau = |t[i+j]-t[i]| <= maxlag are kept in
// enumeration order (segment, i, j) and stably sorted by tau, which is what sortperm over the concatenation of the segments' sorted
// results gives (src/autocov.jl:1-12: the stable sort of (tau, segment, enumeration index)).  The pipeline:
//   1. seg_stats      one workgroup per segment: isequidistant, sum y, var, dot(y,y), the constant-series test -> branch and mode
//   2. lag_sums       equidistant segments: c_j = dot(y[0:n-j], y[j:n]) / divisor, one workgroup per lag, double, fixed order
//   3. row_counts     kept pairs per row (closed form n-i when maxlag is +Inf or NaN), then a 64-bit exclusive scan -> row offsets
//   4. generate       one wave per row: ballot + mbcnt compaction of (tau bits, acf) in enumeration order; AND / OR of all keys
//   5. radix sort     stable LSD, 8-bit digits; passes on which all keys agree (AND == OR on the digit) are skipped.  Each wave
//                     owns a subtile of SUB keys: histogram per (digit, subtile), exclusive scan over digit-major order, scatter with
//                     in-chunk ranks from 8 ballots and per-wave running counters in LDS.  acf travels as the payload.
// tau >= +0 (abs), so its IEEE bits order as unsigned integers; NaN tau is canonicalised to one key that sorts after +Inf (isless).
#include "lpvs_internal.h"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace lpvs {
namespace {

constexpr int kBlock = 256;          // 4 waves
constexpr int kWave = 64;
constexpr int64_t kSub = 8192;       // keys per wave-subtile of the radix sort
constexpr int kScanItems = 16;       // int64 scan: items per thread, kBlock * kScanItems per workgroup
constexpr int64_t kScanTile = (int64_t)kBlock * kScanItems;

int32_t need_device_for_autofun() {
    if (lpvs_device_count() == 0) { set_error("no HIP device visible (the gfx950 path has no CPU fallback)"); return LPVS_EDEVICE; }
    return LPVS_OK;
}

enum : int32_t { MODE_VALUES = 0, MODE_ZEROS = 1, MODE_ONES = 2 };

struct SegStat {
    int32_t equi;   // isequidistant(t) of the segment (src/autocov.jl:112-121)
    int32_t mode;   // MODE_*: the degenerate-series rules
    double var;     // corrected variance (the _autocor divisor)
    double dd;      // dot(y, y)
};

template <class T> struct KeyOf;
template <> struct KeyOf<double> { using K = uint64_t; static constexpr uint64_t nan = 0x7FF8000000000000ull; static constexpr int bits = 64; };
template <> struct KeyOf<float> { using K = uint32_t; static constexpr uint32_t nan = 0x7FC00000u; static constexpr int bits = 32; };

template <class T> __host__ __device__ inline typename KeyOf<T>::K key_of(T tau) {
    typename KeyOf<T>::K k;
    memcpy(&k, &tau, sizeof(T));
    return tau != tau ? KeyOf<T>::nan : k;
}

__host__ __device__ inline double absv(double x) { return __builtin_fabs(x); }
__host__ __device__ inline float absv(float x) { return __builtin_fabsf(x); }

// one step of isequidistant: abs(abs(v[i]-v[i-1]) - d) < 20d*eps() with eps() of Float64 (20d is in the eltype of t)
template <class T> __host__ __device__ inline bool equi_step(T a, T b, T d) {
    const T diff = b - a;
    const T dev = absv(absv(diff) - d);
    const T d20 = (T)20 * d;
    return (double)dev < (double)d20 * DBL_EPSILON;
}

// tau of a pair and whether it is kept (src/autocov.jl:44-45: `tau > maxlag && continue`; NaN maxlag keeps everything)
template <class T> __device__ inline bool keep_pair(T ti, T tj, double maxlag, T *tau) {
    *tau = absv(tj - ti);   // sign bit cleared: +0 for equal times
    return !((double)*tau > maxlag);
}

__device__ inline int64_t seg_of(const int64_t *off, int64_t nseg, int64_t r) {   // largest s with off[s] <= r
    int64_t lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// compensated (double-double) sums of the rounded terms: var(y) and dot(y,y) are their exact sums rounded once (but for rare ties), so
// the autocor divisor does not depend on a summation order
struct DD { double hi, lo; };
__device__ inline DD dd_add(DD a, double b) {   // TwoSum of a.hi + b, the error folded into lo
    const double s = a.hi + b, bb = s - a.hi, e = (a.hi - (s - bb)) + (b - bb);
    return DD{s, a.lo + e};
}
__device__ inline DD dd_add(DD a, DD b) { DD r = dd_add(a, b.hi); r.lo += b.lo; return r; }
__device__ inline DD dd_sq_add(DD a, double x) { return dd_add(a, x * x); }

__device__ inline double block_sum(double v, double *red) {   // fixed tree order: deterministic
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}
__device__ inline double block_sum(DD v, double *red, double *red2) {   // the double-double total, rounded
    const int tid = threadIdx.x;
    red[tid] = v.hi; red2[tid] = v.lo;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const DD r = dd_add(DD{red[tid], red2[tid]}, DD{red[tid + w], red2[tid + w]});
            red[tid] = r.hi; red2[tid] = r.lo;
        }
        __syncthreads();
    }
    const double s = red[0] + red2[0];
    __syncthreads();
    return s;
}

// ---- 1. per-segment statistics ---------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(kBlock) seg_stats_kernel(const T *t, const T *y, const int64_t *off, int32_t kind, SegStat *st) {
    __shared__ double red[kBlock], red2[kBlock];
    const int64_t s = blockIdx.x, o = off[s], n = off[s + 1] - o;
    const int tid = threadIdx.x;
    const T *ts = t + o, *ys = y + o;
    const T d = ts[1] - ts[0];
    int equi = d > (T)0;
    int same = 1;
    DD sy{0.0, 0.0}, syy{0.0, 0.0};
    for (int64_t i = tid; i < n; i += kBlock) {
        const T yi = ys[i];
        if (i >= 2 && equi && !equi_step(ts[i - 1], ts[i], d)) equi = 0;
        if (!(yi == ys[0])) same = 0;
        sy = dd_add(sy, (double)yi);
        syy = dd_sq_add(syy, (double)yi);
    }
    equi = __syncthreads_and(equi);
    same = __syncthreads_and(same);
    const double mean = block_sum(sy, red, red2) / (double)n;
    const double yy = block_sum(syy, red, red2);
    DD sd{0.0, 0.0};
    for (int64_t i = tid; i < n; i += kBlock) sd = dd_sq_add(sd, (double)ys[i] - mean);
    const double ss = block_sum(sd, red, red2);
    if (tid == 0) {
        const T var = (T)(ss / (double)(n - 1)), dd = (T)yy;   // in the eltype of y, as var(y) / dot(y,y) are
        int mode = MODE_VALUES;
        if (kind == LPVS_ACF_COV) {
            if (same || (double)var < DBL_EPSILON) mode = MODE_ZEROS;                       // src/autocov.jl:53-55, :144-146
        } else {
            if ((double)(equi ? dd : var) < DBL_EPSILON) mode = MODE_ONES;                 // src/autocov.jl:96-98, :170-172
        }
        st[s] = SegStat{equi, mode, (double)var, (double)dd};
    }
}

// ---- 2. lag sums of the equidistant branch: one workgroup per (segment, lag j) --------------------------------------------------
template <class T>
__global__ void __launch_bounds__(kBlock) lag_sums_kernel(const T *y, const int64_t *off, int64_t nseg, const SegStat *st,
                                                          int32_t kind, int32_t normalize, double *c) {
    __shared__ double red[kBlock];
    const int64_t r = blockIdx.x, s = seg_of(off, nseg, r);
    const SegStat g = st[s];
    if (!g.equi || g.mode != MODE_VALUES) return;
    const int64_t o = off[s], n = off[s + 1] - o, j = r - o;
    const T *ys = y + o;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n - j; i += kBlock) acc = fma((double)ys[i], (double)ys[i + j], acc);
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double nn = (double)n, nz = normalize ? 1.0 : 0.0;
        c[r] = kind == LPVS_ACF_COV ? acc / (nn - nz * (double)(j - 1))                 // src/autocov.jl:47 (the j-1 of corrected=true)
                                    : acc / ((T)g.dd * (nn - nz * (double)j) / nn);      // src/autocov.jl:90
    }
}

// ---- 3. kept pairs per row --------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(kBlock) row_counts_kernel(const T *t, const int64_t *off, int64_t nseg, int64_t rows, double maxlag,
                                                            int32_t all_kept, int64_t *cnt) {
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    if (r >= rows) return;
    const int64_t s = seg_of(off, nseg, r), m = off[s + 1] - r;   // pairs j = 0 .. m-1 of row r
    if (all_kept) { if (lane == 0) cnt[r] = m; return; }
    const T ti = t[r];
    int64_t k = 0;
    for (int64_t j0 = 0; j0 < m; j0 += kWave) {
        const int64_t j = j0 + lane;
        T tau;
        const bool keep = j < m && keep_pair(ti, t[r + j], maxlag, &tau);
        k += __popcll(__ballot(keep));
    }
    if (lane == 0) cnt[r] = k;
}

// ---- 4. compacting generation --------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(kBlock) generate_kernel(const T *t, const T *y, const int64_t *off, int64_t nseg, int64_t rows,
                                                          const SegStat *st, const double *c, int32_t kind, double maxlag,
                                                          const int64_t *rowoff, typename KeyOf<T>::K *keys, T *vals,
                                                          unsigned long long *kand, unsigned long long *kor) {
    using K = typename KeyOf<T>::K;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const int lane = threadIdx.x % kWave;
    if (r >= rows) return;
    const int64_t s = seg_of(off, nseg, r), m = off[s + 1] - r, o = off[s];
    const SegStat g = st[s];
    const T ti = t[r], yi = y[r], var = (T)g.var;
    int64_t pos = rowoff[r];
    const int64_t end = rowoff[r + 1];
    K a = ~(K)0, b = 0;
    for (int64_t j0 = 0; j0 < m; j0 += kWave) {
        const int64_t j = j0 + lane;
        T tau = 0;
        const bool keep = j < m && keep_pair(ti, t[r + j], maxlag, &tau);
        const unsigned long long bal = __ballot(keep);
        const int64_t p = pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (keep && p < end) {
            T v;
            if (g.mode == MODE_ZEROS) v = (T)0;
            else if (g.mode == MODE_ONES) v = (T)1;
            else if (g.equi) v = (T)c[o + j];                                                  // c_j of the segment
            else if (kind == LPVS_ACF_COV) v = yi * y[r + j];                                 // src/autocov.jl:139
            else v = tau == (T)0 ? (T)1 : (yi * y[r + j]) / var;                             // src/autocov.jl:163, :173-175
            const K k = key_of(tau);
            keys[p] = k;
            vals[p] = v;
            a &= k; b |= k;
        }
        pos += __popcll(bal);
    }
    for (int w = kWave / 2; w > 0; w >>= 1) {
        a &= (K)__shfl_xor((unsigned long long)a, w);
        b |= (K)__shfl_xor((unsigned long long)b, w);
    }
    if (lane == 0 && end > rowoff[r]) {
        atomicAnd(kand, (unsigned long long)a);
        atomicOr(kor, (unsigned long long)b);
    }
}

// ---- int64 exclusive scan (in place) ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) scan_tile_kernel(int64_t *x, int64_t n, int64_t *sums) {
    __shared__ int64_t part[kBlock];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int64_t v[kScanItems], tot = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) { v[k] = base + k < n ? x[base + k] : 0; tot += v[k]; }
    part[threadIdx.x] = tot;
    __syncthreads();
    for (int w = 1; w < kBlock; w <<= 1) {   // Hillis-Steele inclusive scan of the thread totals
        const int64_t add = threadIdx.x >= w ? part[threadIdx.x - w] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - tot;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) { if (base + k < n) x[base + k] = run; run += v[k]; }
    if (threadIdx.x == kBlock - 1 && sums) sums[blockIdx.x] = part[kBlock - 1];
}
__global__ void __launch_bounds__(kBlock) scan_add_kernel(int64_t *x, int64_t n, const int64_t *sums) {
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    const int64_t add = sums[blockIdx.x];
    for (int64_t k = threadIdx.x; k < kScanTile && base + k < n; k += kBlock) x[base + k] += add;
}

int32_t exclusive_scan(int64_t *x, int64_t n, hipStream_t s) {
    if (n <= 0) return LPVS_OK;
    const int64_t tiles = ceil_div(n, kScanTile);
    if (tiles == 1) {
        scan_tile_kernel<<<1, kBlock, 0, s>>>(x, n, nullptr);
        LPVS_HIP(hipGetLastError());
        return LPVS_OK;
    }
    DevBuf sums;
    LPVS_TRY(sums.alloc(sizeof(int64_t) * (size_t)tiles));
    scan_tile_kernel<<<(unsigned)tiles, kBlock, 0, s>>>(x, n, sums.as<int64_t>());
    LPVS_HIP(hipGetLastError());
    LPVS_TRY(exclusive_scan(sums.as<int64_t>(), tiles, s));
    scan_add_kernel<<<(unsigned)tiles, kBlock, 0, s>>>(x, n, sums.as<int64_t>());
    LPVS_HIP(hipGetLastError());
    DrainOnExit drain(s);   // sums goes back to the pool once the add has run
    return LPVS_OK;
}

// ---- 5. stable LSD radix sort ---------------------------------------------------------------------------------------------------------
template <class K>
__global__ void __launch_bounds__(kBlock) radix_hist_kernel(const K *keys, int64_t P, int64_t nsub, int shift, int64_t *hist) {
    __shared__ uint32_t h[kBlock / kWave][256];
    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int64_t sub = (int64_t)blockIdx.x * (kBlock / kWave) + w;
    for (int d = lane; d < 256; d += kWave) h[w][d] = 0;
    __syncthreads();
    if (sub < nsub) {
        const int64_t lo = sub * kSub, hi = lo + kSub < P ? lo + kSub : P;
        for (int64_t i = lo + lane; i < hi; i += kWave) atomicAdd(&h[w][(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (sub < nsub)
        for (int d = lane; d < 256; d += kWave) hist[(int64_t)d * nsub + sub] = h[w][d];
}

template <class K, class V>
__global__ void __launch_bounds__(kBlock) radix_scatter_kernel(const K *kin, const V *vin, int64_t P, int64_t nsub, int shift,
                                                               const int64_t *offs, K *kout, V *vout) {
    __shared__ int64_t base[kBlock / kWave][256];
    __shared__ uint32_t run[kBlock / kWave][256];
    const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int64_t sub = (int64_t)blockIdx.x * (kBlock / kWave) + w;
    if (sub >= nsub) return;   // waves are independent: no workgroup barrier below
    for (int d = lane; d < 256; d += kWave) { base[w][d] = offs[(int64_t)d * nsub + sub]; run[w][d] = 0; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int64_t lo = sub * kSub, hi = lo + kSub < P ? lo + kSub : P;
    for (int64_t c = lo; c < hi; c += kWave) {
        const int64_t i = c + lane;
        const bool act = i < hi;
        K k = 0;
        V v = 0;
        if (act) { k = kin[i]; v = vin[i]; }
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        unsigned long long same = __ballot(act);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bb = __ballot(act && ((d >> b) & 1u));
            same &= ((d >> b) & 1u) ? bb : ~bb;
        }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        uint32_t before = 0;
        if (act) before = run[w][d];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (act && rank == 0) run[w][d] = before + (uint32_t)__popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (act) {
            const int64_t p = base[w][d] + before + rank;
            if (p < P) { kout[p] = k; vout[p] = v; }
        }
    }
}

// ---- thread-local phase times of the last call -----------------------------------------------------------------------------------------
thread_local double g_timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};

template <class T> int32_t isequidistant_host(const T *t, int64_t N) {
    const T d = t[1] - t[0];
    if (!(d > (T)0)) return 0;
    for (int64_t i = 2; i < N; ++i)
        if (!equi_step(t[i - 1], t[i], d)) return 0;
    return 1;
}

template <class T> int32_t isequidistant_impl(const T *t, int64_t N, int32_t *eq) {
    if (!t || !eq) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (N < 2) { set_error("isequidistant needs at least 2 samples, got %lld", (long long)N); return LPVS_EARGUMENT; }
    const int owner = device_of_ptr(t);
    if (owner < 0) { *eq = isequidistant_host(t, N); return LPVS_OK; }
    // device t: the statistics kernel of one segment [0, N); y = t (its values are not used)
    LPVS_HIP(hipSetDevice(owner));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    DevBuf off, st;
    LPVS_TRY(off.alloc(2 * sizeof(int64_t)));
    LPVS_TRY(st.alloc(sizeof(SegStat)));
    DrainOnExit drain(sh.s);
    const int64_t ho[2] = {0, N};
    LPVS_TRY(copy_to_device(off.p, ho, sizeof(ho), sh.s));
    seg_stats_kernel<T><<<1, kBlock, 0, sh.s>>>(t, t, off.as<int64_t>(), LPVS_ACF_COV, st.as<SegStat>());
    LPVS_HIP(hipGetLastError());
    SegStat g;
    LPVS_TRY(copy_from_device(&g, st.p, sizeof(g), sh.s));
    *eq = g.equi;
    return LPVS_OK;
}

template <class T>
int32_t autofun_impl(int32_t kind, const T *t, const T *y, const int64_t *seg_off, int64_t nseg, double maxlag, int32_t normalize,
                     int32_t device, T *tau_out, T *acf_out, int64_t capacity, int64_t *count) {
    using K = typename KeyOf<T>::K;
    // ---- arguments (before any device is needed)
    if (kind != LPVS_ACF_COV && kind != LPVS_ACF_COR) { set_error("kind must be LPVS_ACF_COV or LPVS_ACF_COR, got %d", kind); return LPVS_EARGUMENT; }
    if (!t || !y || !seg_off || !count) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (nseg < 1) { set_error("nseg must be positive"); return LPVS_EARGUMENT; }
    if ((tau_out == nullptr) != (acf_out == nullptr)) { set_error("tau_out and acf_out must both be given or both be NULL (count only)"); return LPVS_EARGUMENT; }
    if (seg_off[0] != 0) { set_error("seg_off[0] must be 0"); return LPVS_EARGUMENT; }
    int64_t all_pairs = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t n = seg_off[s + 1] - seg_off[s];
        if (n < 2) { set_error("segment %lld has %lld samples: at least 2 are needed (isequidistant reads t[2])", (long long)s, (long long)n); return LPVS_EARGUMENT; }
        all_pairs += n * (n + 1) / 2;
    }
    const int64_t rows = seg_off[nseg];
    const int32_t all_kept = std::isnan(maxlag) || (std::isinf(maxlag) && maxlag > 0);
    LPVS_TRY(need_device_for_autofun());
    LPVS_HIP(hipSetDevice(device));

    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    const hipStream_t s = sh.s;
    Events<6> ev;
    for (auto &x : ev.e) LPVS_HIP(hipEventCreate(&x));
    Staged<T> dt, dy;
    DevBuf doff, dst, dc, dcnt, dbits, hist, k0, v0, k1, v1;
    DrainOnExit drain(s);
    LPVS_HIP(hipEventRecord(ev.e[0], s));
    LPVS_TRY(dt.set(t, rows, device, s));
    LPVS_TRY(dy.set(y, rows, device, s));
    LPVS_TRY(doff.alloc(sizeof(int64_t) * (size_t)(nseg + 1)));
    LPVS_TRY(copy_to_device(doff.p, seg_off, sizeof(int64_t) * (size_t)(nseg + 1), s));
    LPVS_TRY(dst.alloc(sizeof(SegStat) * (size_t)nseg));
    LPVS_TRY(dcnt.alloc(sizeof(int64_t) * (size_t)(rows + 1)));
    const int64_t *off = doff.as<int64_t>();

    // ---- 1 + 3: statistics, kept pairs per row, row offsets
    seg_stats_kernel<T><<<(unsigned)nseg, kBlock, 0, s>>>(dt.p, dy.p, off, kind, dst.as<SegStat>());
    LPVS_HIP(hipGetLastError());
    const unsigned row_blocks = (unsigned)ceil_div(rows, kBlock / kWave);
    LPVS_HIP(hipMemsetAsync(dcnt.as<int64_t>() + rows, 0, sizeof(int64_t), s));
    row_counts_kernel<T><<<row_blocks, kBlock, 0, s>>>(dt.p, off, nseg, rows, maxlag, all_kept, dcnt.as<int64_t>());
    LPVS_HIP(hipGetLastError());
    LPVS_TRY(exclusive_scan(dcnt.as<int64_t>(), rows + 1, s));
    int64_t P = 0;
    LPVS_TRY(copy_from_device(&P, dcnt.as<int64_t>() + rows, sizeof(P), s));
    LPVS_HIP(hipEventRecord(ev.e[1], s));
    *count = P;
    if (all_kept && P != all_pairs) { set_error("internal: %lld kept pairs of %lld", (long long)P, (long long)all_pairs); return LPVS_EASSERT; }
    if (!tau_out) return LPVS_OK;   // count only
    if (capacity < P) { set_error("capacity %lld < %lld pairs", (long long)capacity, (long long)P); return LPVS_EARGUMENT; }
    if (P == 0) return LPVS_OK;

    // ---- memory: outputs and scratch must fit, or LPVS_ENOMEM (never a fault)
    const bool dev_out = device_of_ptr(tau_out) == device && device_of_ptr(acf_out) == device;
    const int64_t nsub = ceil_div(P, kSub);
    const size_t pair_bytes = (sizeof(K) + sizeof(T)) * (size_t)P;
    const size_t need = (dev_out ? 1 : 2) * pair_bytes + sizeof(int64_t) * (size_t)(256 * nsub) * 2 + sizeof(double) * (size_t)rows;
    size_t fr = 0, tot = 0;
    LPVS_HIP(hipMemGetInfo(&fr, &tot));
    const size_t avail = fr + pool_cached_bytes(device);
    if (need > avail) {
        set_error("autocov/autocor: %lld pairs need %.2f GB of device memory (%s), %.2f GB are free", (long long)P, need / 1e9,
                  dev_out ? "scratch" : "outputs and scratch", avail / 1e9);
        return LPVS_ENOMEM;
    }
    LPVS_TRY(dc.alloc(sizeof(double) * (size_t)rows));
    LPVS_TRY(dbits.alloc(2 * sizeof(unsigned long long)));
    K *ka, *kb;
    T *va, *vb;
    if (dev_out) { ka = reinterpret_cast<K *>(tau_out); va = acf_out; }
    else {
        LPVS_TRY(k0.alloc(sizeof(K) * (size_t)P)); LPVS_TRY(v0.alloc(sizeof(T) * (size_t)P));
        ka = k0.as<K>(); va = v0.as<T>();
    }
    LPVS_TRY(k1.alloc(sizeof(K) * (size_t)P)); LPVS_TRY(v1.alloc(sizeof(T) * (size_t)P));
    kb = k1.as<K>(); vb = v1.as<T>();
    LPVS_TRY(hist.alloc(sizeof(int64_t) * (size_t)(256 * nsub)));

    // ---- 2 + 4: lag sums of the equidistant segments, generation in enumeration order
    lag_sums_kernel<T><<<(unsigned)rows, kBlock, 0, s>>>(dy.p, off, nseg, dst.as<SegStat>(), kind, normalize, dc.as<double>());
    LPVS_HIP(hipGetLastError());
    const unsigned long long init_bits[2] = {~0ull, 0ull};
    LPVS_HIP(hipMemcpyAsync(dbits.p, init_bits, sizeof(init_bits), hipMemcpyHostToDevice, s));
    unsigned long long *kand = dbits.as<unsigned long long>(), *kor = kand + 1;
    generate_kernel<T><<<row_blocks, kBlock, 0, s>>>(dt.p, dy.p, off, nseg, rows, dst.as<SegStat>(), dc.as<double>(), kind, maxlag,
                                                      dcnt.as<int64_t>(), ka, va, kand, kor);
    LPVS_HIP(hipGetLastError());
    unsigned long long hb[2];
    LPVS_TRY(copy_from_device(hb, dbits.p, sizeof(hb), s));
    LPVS_HIP(hipEventRecord(ev.e[2], s));

    // ---- 5: radix sort over the digits on which the keys differ
    const unsigned long long differ = hb[0] ^ hb[1];
    const unsigned sub_blocks = (unsigned)ceil_div(nsub, kBlock / kWave);
    int passes = 0;
    for (int shift = 0; shift < KeyOf<T>::bits; shift += 8) {
        if (((differ >> shift) & 255ull) == 0) continue;
        radix_hist_kernel<K><<<sub_blocks, kBlock, 0, s>>>(ka, P, nsub, shift, hist.as<int64_t>());
        LPVS_HIP(hipGetLastError());
        LPVS_TRY(exclusive_scan(hist.as<int64_t>(), 256 * nsub, s));
        radix_scatter_kernel<K, T><<<sub_blocks, kBlock, 0, s>>>(ka, va, P, nsub, shift, hist.as<int64_t>(), kb, vb);
        LPVS_HIP(hipGetLastError());
        std::swap(ka, kb); std::swap(va, vb);
        ++passes;
    }
    LPVS_HIP(hipEventRecord(ev.e[3], s));

    // ---- out: tau is the key (tau >= +0), acf the payload
    if (reinterpret_cast<T *>(ka) != tau_out) {
        LPVS_HIP(hipMemcpyAsync(tau_out, ka, sizeof(K) * (size_t)P, dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDefault, s));
        LPVS_HIP(hipMemcpyAsync(acf_out, va, sizeof(T) * (size_t)P, dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDefault, s));
    }
    LPVS_HIP(hipEventRecord(ev.e[4], s));
    LPVS_HIP(hipStreamSynchronize(s));
    float ms[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) LPVS_HIP(hipEventElapsedTime(&ms[k], ev.e[k], ev.e[k + 1]));
    // [0] stats + counts + scan, [1] lag sums + generation, [2] sort, [3] copy out, [4] total, [5] pairs, [6] sort passes, [7] key bytes
    g_timing[0] = ms[0]; g_timing[1] = ms[1]; g_timing[2] = ms[2]; g_timing[3] = ms[3];
    g_timing[4] = (double)ms[0] + ms[1] + ms[2] + ms[3]; g_timing[5] = (double)P; g_timing[6] = passes; g_timing[7] = sizeof(K);
    return LPVS_OK;
}

}  // namespace
}  // namespace lpvs

using namespace lpvs;

extern "C" {

int32_t lpvs_isequidistant_f64(const double *t, int64_t N, int32_t *equidistant) { return isequidistant_impl(t, N, equidistant); }
int32_t lpvs_isequidistant_f32(const float *t, int64_t N, int32_t *equidistant) { return isequidistant_impl(t, N, equidistant); }

int32_t lpvs_autofun_f64(int32_t kind, const double *t, const double *y, const int64_t *seg_off, int64_t nseg, double maxlag,
                         int32_t normalize, int32_t device, double *tau_out, double *acf_out, int64_t capacity, int64_t *count) {
    try {
        return autofun_impl(kind, t, y, seg_off, nseg, maxlag, normalize, device, tau_out, acf_out, capacity, count);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_autofun_f32(int32_t kind, const float *t, const float *y, const int64_t *seg_off, int64_t nseg, double maxlag,
                         int32_t normalize, int32_t device, float *tau_out, float *acf_out, int64_t capacity, int64_t *count) {
    try {
        return autofun_impl(kind, t, y, seg_off, nseg, maxlag, normalize, device, tau_out, acf_out, capacity, count);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_autofun_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_timing, 8);
}

}  // extern "C"
