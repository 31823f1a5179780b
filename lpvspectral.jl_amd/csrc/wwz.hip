// wwz.hip -- Foster's weighted wavelet Z-transform of non-uniformly sampled signals (wwz; hand-written HIP, gfx950; the definition:
// include/lpvspectral.h g8; the decisions: wwz_plan.h).
//
// A cell (frequency f_k, time tau_j) is the floating-mean fit of g4 of the samples with tau_j - radius_k <= t <= tau_j + radius_k under the
// weights W g, g = exp(-a_k (t - tau_j)^2).  Per cell, with phases phi = 2 pi f_k t of the exact products (origin t = 0: shared by every
// time of a frequency):
//   SW = sum Wg, SW2 = sum (Wg)^2, C, S, C2, S2 = sum Wg {cos, sin, cos 2, sin 2} phi,   Y, YY, YC, YS = sum Wg yc {1, yc, cos phi, sin phi}
// (yc = y less the record's weighted mean), all with the UNNORMALISED W g; the epilogue divides by SW.
//
// RANGES: wwz_ranges_kernel, one binary search per edge, edges = #{t < a - r}, #{t <= b + r}: the cells (a = b = tau_j, r = radius_k) and
// the (group, tile) pairs of the work list (a, b = the group's first and last time, r = the tile's largest radius).
//
// SUMS: wwz_sums_kernel<TT, TS>.  The family's workgroup -- 64 frequencies x 4 sample lanes, 256 samples staged through LDS -- walks one
// item of the work list: a group of TT adjacent times, a tile of frequencies, one slab of the samples the pair reaches.  Per (sample,
// frequency) ONE sincospi (lomb_sincos) and the double angle serve the thread's TT times; per time the thread tests its own
// lo <= t <= hi, evaluates one exp and adds 6 + 4 TS terms.  Every accumulator has a static index (TT and TS are template parameters, the
// loops over them unrolled).  FIXED ORDER: lane = the sample's ABSOLUTE index mod 4, stages at absolute multiples of 256, slabs at
// absolute multiples of the slab length; a sample outside a cell is skipped by a predicate, never added as a zero.  What is added behind
// a cell, and in which order, depends on that cell's samples and on N alone -- not on the group, the list of times, or the other signals.
//
// EPILOGUE: wwz_epilogue_kernel, one thread per (frequency, time, signal): lomb_pairwise over the slabs the CELL touches (counted from
// its own first slab), the division by SW, lomb_fit with fit_mean, and the rules of g8 for empty cells, Neff <= 3 and exact fits.
#include "lpvs_internal.h"
#include "lomb_device.h"
#include "wwz_plan.h"

namespace lpvs {
namespace {

// t finite and non-decreasing: flags |= 1, |= 8 (the rule of lomb.hip's time windows)
__global__ void __launch_bounds__(256) wwz_sorted_kernel(const double *__restrict__ t, int64_t N, int *__restrict__ flags) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int bad = 0;
    if (!(fabs(t[n]) < 1.0 / 0.0)) bad |= 1;
    if (n + 1 < N && t[n] > t[n + 1]) bad |= 8;
    if (bad) atomicOr(flags, bad);
}

// pair q = j nr + k: edges[2 q] = #{t < a[j] - r[k]}, edges[2 q + 1] = #{t <= b[j] + r[k]}; both edges formed in double as written
__global__ void __launch_bounds__(256)
wwz_ranges_kernel(const double *__restrict__ t, int64_t N, const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ r, int64_t nr,
                  int64_t npairs, int64_t *__restrict__ edges) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * npairs) return;
    const bool upper = e & 1;
    const int64_t q = e >> 1, j = q / nr, k = q - j * nr;
    const double v = upper ? b[j] + r[k] : a[j] - r[k];
    int64_t lo = 0, hi = N;                                                // the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const double tv = t[mid];
        if (upper ? tv <= v : tv < v) lo = mid + 1; else hi = mid;
    }
    edges[e] = lo;
}

// accumulators of a thread: acc[tt NR + {0 .. 5}] = SW, SW2, C, S, C2, S2 of its time tt; acc[tt NR + 6 + 4 c + {0 .. 3}] = Y, YY, YC, YS of signal c
template <int TT, int TS>
__device__ inline void wwz_walk_stage(double fv, double ak, const double *tau, const double *lo, const double *hi, const double *st, const double *sw,
                                      const double (*sy)[LB_STAGE], int i0, int i1, int lane, double *acc) {
    constexpr int NR = kWwzSharedSums + kWwzSignalSums * TS;
    for (int i = i0 + ((lane - i0) & (LB_LANES - 1)); i < i1; i += LB_LANES) {
        const double tv = st[i];
        bool in[TT], any = false;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) { in[tt] = lo[tt] <= tv && tv <= hi[tt]; any = any || in[tt]; }
        if (!any) continue;
        double sn, cs;
        lomb_sincos(fv, tv, &sn, &cs);
        const double c2 = fma(cs, cs, -(sn * sn)), s2 = 2.0 * (sn * cs), wv = sw[i];
        double yc[TS];
#pragma unroll
        for (int c = 0; c < TS; ++c) yc[c] = sy[c][i];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            if (!in[tt]) continue;
            const double d = tv - tau[tt];
            const double wg = wv * exp(-(ak * (d * d)));
            double *a = acc + tt * NR;
            a[0] = a[0] + wg;
            a[1] = fma(wg, wg, a[1]);
            a[2] = fma(wg, cs, a[2]);
            a[3] = fma(wg, sn, a[3]);
            a[4] = fma(wg, c2, a[4]);
            a[5] = fma(wg, s2, a[5]);
#pragma unroll
            for (int c = 0; c < TS; ++c) {
                const double v = wg * yc[c];
                a[6 + 4 * c] = a[6 + 4 * c] + v;
                a[7 + 4 * c] = fma(v, yc[c], a[7 + 4 * c]);
                a[8 + 4 * c] = fma(v, cs, a[8 + 4 * c]);
                a[9 + 4 * c] = fma(v, sn, a[9 + 4 * c]);
            }
        }
    }
}

// workgroup = (item of the work list) x (block of TS signals).  part[((item rows + row) TT + tt) 64 + fl]: rows 0 .. 5 (written by signal
// block 0), then 6 + 4 c + {0 .. 3} of every signal c
template <int TT, int TS>
__global__ void __launch_bounds__(256) wwz_sums_kernel(const WwzArgs A, double *__restrict__ part) {
    constexpr int NR = kWwzSharedSums + kWwzSignalSums * TS, NA = TT * NR;
    static_assert(NA <= kWwzMaxAcc, "the accumulators of a thread");
    __shared__ double st[LB_STAGE], sw[LB_STAGE], sy[TS][LB_STAGE];
    __shared__ double red[LB_LANES][LB_LANES][LB_TF];                      // [accumulator of the group of four][sample lane][frequency]
    const int fl = threadIdx.x % LB_TF, lane = threadIdx.x / LB_TF;
    const WwzItem it = A.items[blockIdx.x];
    const int64_t k = (int64_t)it.tile * LB_TF + fl;
    const bool live = k < A.Nf;
    const int c0 = blockIdx.y * TS, ns = A.ns;
    // a lane past the last frequency has the radius -1: lo > hi, so no sample is ever inside
    const double fv = live ? A.f[k] : 0.0, ak = live ? A.decay[k] : 0.0, rk = live ? A.radius[k] : -1.0;
    double tau[TT], lo[TT], hi[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        tau[tt] = A.tau[(int64_t)it.group * TT + tt];
        lo[tt] = tau[tt] - rk;
        hi[tt] = tau[tt] + rk;
    }
    double m[TS];
#pragma unroll
    for (int c = 0; c < TS; ++c) m[c] = A.mean && c0 + c < ns ? A.mean[c0 + c] : 0.0;
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    for (int64_t base = it.first - it.first % LB_STAGE; base < it.last; base += LB_STAGE) {
        const int i0 = (int)(it.first > base ? it.first - base : 0), i1 = (int)(it.last - base < LB_STAGE ? it.last - base : LB_STAGE);
        __syncthreads();                                                   // the previous stage has been walked
        if ((int)threadIdx.x >= i0 && (int)threadIdx.x < i1) {
            const int64_t n = base + threadIdx.x;
            st[threadIdx.x] = A.t[n];
            sw[threadIdx.x] = A.W ? A.W[n] : 1.0;
#pragma unroll
            for (int c = 0; c < TS; ++c) sy[c][threadIdx.x] = c0 + c < ns ? A.y[(int64_t)(c0 + c) * A.N + n] - m[c] : 0.0;
        }
        __syncthreads();
        wwz_walk_stage<TT, TS>(fv, ak, tau, lo, hi, st, sw, sy, i0, i1, lane, acc);
    }
    // the four lanes of every accumulator as (0 + 1) + (2 + 3), four accumulators at a time through LDS
    double *o = part + (int64_t)blockIdx.x * A.rows * (TT * LB_TF) + fl;
#pragma unroll
    for (int a0 = 0; a0 < NA; a0 += LB_LANES) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LB_LANES; ++q)
            if (a0 + q < NA) red[q][lane][fl] = acc[a0 + q];
        __syncthreads();
        if (lane == 0 && live) {
#pragma unroll
            for (int q = 0; q < LB_LANES; ++q) {
                if (a0 + q >= NA) continue;
                const int tt = (a0 + q) / NR, r = (a0 + q) % NR;
                const double v = lomb_lane_sum(red[q], fl);
                if (r < kWwzSharedSums) { if (blockIdx.y == 0) o[((int64_t)r * TT + tt) * LB_TF] = v; }
                else if (c0 + (r - kWwzSharedSums) / kWwzSignalSums < ns) o[((int64_t)(r + kWwzSignalSums * c0) * TT + tt) * LB_TF] = v;
            }
        }
    }
}

// one thread per (frequency k, time j, signal c): e = (c Ntau + j) Nf + k.  The cell's slabs are added by lomb_pairwise, counted from the
// cell's own first slab.  Planes power, amplitude, wwz (and coef: a, b, c) at e; neff, count, empty at j Nf + k (written by signal 0).
__global__ void __launch_bounds__(256)
wwz_epilogue_kernel(const WwzArgs A, const double *__restrict__ part, const int64_t *__restrict__ cell_edges, int center, double *__restrict__ power,
                    double *__restrict__ amplitude, double *__restrict__ wwz, double *__restrict__ neff_out, double *__restrict__ coef, int64_t *__restrict__ count_out,
                    int32_t *__restrict__ empty_out, int *__restrict__ flags, unsigned long long *__restrict__ counters) {
    const int64_t total = A.Nf * A.Ntau * A.ns, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t k = e % A.Nf, j = (e / A.Nf) % A.Ntau, cell = j * A.Nf + k;
    const int c = (int)(e / (A.Nf * A.Ntau));
    const int64_t start = cell_edges[2 * cell], stop = cell_edges[2 * cell + 1], count = stop > start ? stop - start : 0;
    double sum[kWwzSharedSums + kWwzSignalSums];
#pragma unroll
    for (int r = 0; r < kWwzSharedSums + kWwzSignalSums; ++r) sum[r] = 0.0;
    if (count > 0) {
        const int64_t L = A.slab_samples, s0 = start / L, nslab = (stop - 1) / L - s0 + 1;
        const int p = A.pos[j], TT = A.TT;
        const int64_t pair = (int64_t)(p / TT) * A.ftiles + k / LB_TF, stride = A.rows * (TT * LB_TF);
        const int64_t i0 = A.offset[pair] + (s0 - A.first_slab[pair]);
        if (s0 < A.first_slab[pair] || i0 + nslab > A.offset[pair + 1]) { atomicOr(flags, 16); return; }   // (a cell lies inside its pair: wwz_plan.h)
        const double *src = part + i0 * stride + (int64_t)(p % TT) * LB_TF + k % LB_TF;
#pragma unroll
        for (int r = 0; r < kWwzSharedSums + kWwzSignalSums; ++r) {
            const int row = r < kWwzSharedSums ? r : r + kWwzSignalSums * c;
            sum[r] = lomb_pairwise(src + (int64_t)row * (TT * LB_TF), stride, nslab);
        }
    }
    const double sw = sum[0], sw2 = sum[1];
    const bool live = count > 0 && sw > 0.0 && sw2 > 0.0;
    const double neff = live ? (sw / sw2) * sw : 0.0;
    if (c == 0) {
        if (count > 0 && !(fabs(sw) < 1.0 / 0.0)) atomicOr(flags, 4);
        neff_out[cell] = neff;
        count_out[cell] = count;
        empty_out[cell] = live ? 0 : 1;
        if (!live) atomicAdd(&counters[0], 1ull);
    }
    LombFit r = {0.0, 0.0, 0.0, 0.0, false};
    double z = 0.0;
    if (live) {
        const double C = sum[2] / sw, S = sum[3] / sw, C2 = sum[4] / sw, S2 = sum[5] / sw;
        const double Y = sum[6] / sw, YY = sum[7] / sw, YC = sum[8] / sw, YS = sum[9] / sw;
        const double removed = center ? A.mean[c] : 0.0;
        const double R = fma(removed, fma(2.0, Y, removed), YY);           // sum w y^2 of the signal as given: YY + 2 m Y + m^2
        r = lomb_fit(C, S, C2, S2, YC, YS, Y, YY, R, removed, 1, center, 0, (double)count);
        if (r.degenerate) {
            if (c == 0) atomicAdd(&counters[1], 1ull);
        } else {
            const double noise = lomb_yy_noise((double)count, center != 0, true, R, YY), YYm = fma(-Y, Y, YY);
            if (neff > 3.0 && YYm > noise) {
                const double p = r.pw * YYm, rest = YYm - p;
                z = rest > noise ? ((neff - 3.0) * p) / (2.0 * rest) : 1.0 / 0.0;
            }
        }
    }
    power[e] = r.pw;
    amplitude[e] = hypot(r.a, r.b);
    wwz[e] = z;
    if (coef) { coef[e] = r.a; coef[total + e] = r.b; coef[2 * total + e] = r.c; }
}

}  // namespace

// flags_dev |= 1: a non-finite t, |= 8: t decreases somewhere (not zeroed here: it follows launch_lomb_scan)
int32_t launch_wwz_sorted(const double *t, int64_t N, int *flags_dev, hipStream_t s) {
    hipLaunchKernelGGL(wwz_sorted_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, t, N, flags_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// edges[2 (j nr + k) + {0, 1}] = #{t < a[j] - r[k]}, #{t <= b[j] + r[k]}, j < na, k < nr
int32_t launch_wwz_ranges(const double *t, int64_t N, const double *a, const double *b, int64_t na, const double *r, int64_t nr, int64_t *edges, hipStream_t s) {
    hipLaunchKernelGGL(wwz_ranges_kernel, dim3((unsigned)ceil_div(2 * na * nr, 256)), dim3(256), 0, s, t, N, a, b, r, nr, na * nr, edges);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_wwz_sums(const WwzArgs &A, int ts, double *part, hipStream_t s) {
    if (A.nitems == 0) return LPVS_OK;
    const dim3 grid((unsigned)A.nitems, (unsigned)ceil_div(A.ns, ts));
    const int key = A.TT * 10 + ts;
    switch (key) {
    case 41: hipLaunchKernelGGL((wwz_sums_kernel<4, 1>), grid, dim3(256), 0, s, A, part); break;
    case 21: hipLaunchKernelGGL((wwz_sums_kernel<2, 1>), grid, dim3(256), 0, s, A, part); break;
    case 11: hipLaunchKernelGGL((wwz_sums_kernel<1, 1>), grid, dim3(256), 0, s, A, part); break;
    case 24: hipLaunchKernelGGL((wwz_sums_kernel<2, 4>), grid, dim3(256), 0, s, A, part); break;
    case 14: hipLaunchKernelGGL((wwz_sums_kernel<1, 4>), grid, dim3(256), 0, s, A, part); break;
    default: set_error("wwz: no sums kernel for %d times and %d signals per thread", A.TT, ts); return LPVS_EUNSUPPORTED;
    }
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// counters[2] = {empty cells, degenerate cells}: zeroed here
int32_t launch_wwz_epilogue(const WwzArgs &A, const double *part, const int64_t *cell_edges, bool center, double *power, double *amplitude, double *wwz,
                            double *neff, double *coef, int64_t *count_out, int32_t *empty_out, int *flags_dev, unsigned long long *counters, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(wwz_epilogue_kernel, dim3((unsigned)ceil_div(A.Nf * A.Ntau * A.ns, 256)), dim3(256), 0, s, A, part, cell_edges, center ? 1 : 0, power, amplitude,
                       wwz, neff, coef, count_out, empty_out, flags_dev, counters);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace lpvs
