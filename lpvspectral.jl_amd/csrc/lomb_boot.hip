// lomb_boot.hip -- the bootstrap of the Lomb-Scargle periodogram (lombscargle_bootstrap; hand-written HIP, gfx950).
//
// Resample b of the record has y*_b[i] = y[pi_b(i)]; t and the weights stay where they are, so C, S, C2, S2 are those of the observed
// record (lomb.hip, once) and only YC, YS and three moments differ per resample.
//
// INDICES.  pi_b(i) = (u N) >> 64 with the 64-bit word u of Philox4x32-10, key = the seed, counter = (b, i >> 1): sample 2p takes
// (w0 << 32) | w1, sample 2p + 1 takes (w2 << 32) | w3.  pi < N by construction: no gather leaves y.  They are REGENERATED wherever they
// are consumed (the moments, every tile of frequencies of the bootstrap sums); no array of B x N indices or values is kept.
//
// MOMENTS (lomb_boot_moments_kernel): a workgroup per resample; thread j adds the sample pairs j, j + 256, ... in ascending order, then
// the tree over the threads: first the weighted mean, then Y, YY of the centred resample and R = sum w y*^2.
//
// BOOTSTRAP SUMS (lomb_boot_kernel<TS>): a workgroup = 64 frequencies x 4 sample lanes (as lomb_direct_kernel), one slab of samples, one
// block of TS resamples.  256 samples are staged at a time: t and, per resample, w (y[pi] - m) laid out [sample][TS], so that the walk
// reads a sample's TS values with wide broadcast loads.  The walk: one sincospi per (sample, frequency), 2 TS fused multiply-adds into
// 2 TS register accumulators.  Lanes are added as (0 + 1) + (2 + 3), slabs by the pairwise tree of lomb_pairwise.  Rows of a partial
// block beyond the chunk are computed on zeros and never written.
//
// EPILOGUE + MAXIMUM (lomb_boot_epilogue_kernel): a workgroup per resample, threads stride the frequencies: lomb_fit as it is, the
// optional store of the column, and a tree over (value, index) with ties to the lower index.
//
// Every order of additions depends on N and Nf alone: not on B, row0, the chunk, or whether the columns are stored.
#include "lpvs_internal.h"
#include "lomb_boot_plan.h"
#include "lomb_device.h"
#include "philox.h"

namespace lpvs {
namespace {

// pi_b(2p), pi_b(2p + 1)
__device__ inline void boot_index_pair(uint64_t seed, uint64_t b, uint64_t pair, uint64_t N, uint64_t *i0, uint64_t *i1) {
    const U4 u = philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)pair, (uint32_t)(pair >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
    *i0 = __umul64hi(((uint64_t)u.w[0] << 32) | u.w[1], N);
    *i1 = __umul64hi(((uint64_t)u.w[2] << 32) | u.w[3], N);
}

// ---- moments: workgroup = one resample ---------------------------------------------------------------------------------------------------
// mean[r] = sum w y*; mom[4 r + {0, 1, 2}] = Y, YY of the resample less m (m = mean[r] if center, else 0) and R = sum w y*^2
__global__ void __launch_bounds__(256)
lomb_boot_moments_kernel(const double *__restrict__ y, const double *__restrict__ w, int64_t N, uint64_t seed, int64_t row0, int center, double *__restrict__ mean,
                         double *__restrict__ mom) {
    __shared__ double red[256];
    const int64_t r = blockIdx.x, npairs = (N + 1) / 2;
    const uint64_t b = (uint64_t)(row0 + r);
    double s = 0.0;
    for (int64_t p = threadIdx.x; p < npairs; p += 256) {
        uint64_t i0, i1;
        boot_index_pair(seed, b, (uint64_t)p, (uint64_t)N, &i0, &i1);
        s = fma(w[2 * p], y[i0], s);
        if (2 * p + 1 < N) s = fma(w[2 * p + 1], y[i1], s);
    }
    const double mu = lomb_block_sum(s, red);
    const double m = center ? mu : 0.0;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t p = threadIdx.x; p < npairs; p += 256) {
        uint64_t i0, i1;
        boot_index_pair(seed, b, (uint64_t)p, (uint64_t)N, &i0, &i1);
        {
            const double yr = y[i0], yc = yr - m, v = w[2 * p] * yc;
            s1 = s1 + v; s2 = fma(v, yc, s2); s3 = fma(w[2 * p] * yr, yr, s3);
        }
        if (2 * p + 1 < N) {
            const double yr = y[i1], yc = yr - m, v = w[2 * p + 1] * yc;
            s1 = s1 + v; s2 = fma(v, yc, s2); s3 = fma(w[2 * p + 1] * yr, yr, s3);
        }
    }
    const double Y = lomb_block_sum(s1, red), YY = lomb_block_sum(s2, red), R = lomb_block_sum(s3, red);
    if (threadIdx.x == 0) {
        mean[r] = mu;
        mom[4 * r] = Y; mom[4 * r + 1] = YY; mom[4 * r + 2] = R;
    }
}

// ---- bootstrap sums: workgroup (tile of 64 frequencies x block of TS resamples, slab of samples) --------------------------------------------
// r0: the chunk's first resample counted from row0, count: its resamples; part[((slab 2 count) + 2 j + {0, 1}) Nf + k] = YC, YS of resample
// r0 + j.  mean: per resample counted from row0, or nullptr (nothing is removed).
template <int TS>
__global__ void __launch_bounds__(256)
lomb_boot_kernel(const double *__restrict__ t, const double *__restrict__ w, const double *__restrict__ y, int64_t N, uint64_t seed, int64_t row0, int64_t r0,
                 int64_t count, const double *__restrict__ mean, const double *__restrict__ f, int64_t Nf, int64_t ftiles, int64_t slab_samples,
                 double *__restrict__ part) {
    constexpr int NA = 2 * TS, HALF = TS / 2, RED = 8;                       // accumulators; resamples a staging thread draws; accumulators per round of the lane sum
    static_assert(TS % 2 == 0 && NA % RED == 0, "TS");
    __shared__ double st[LB_STAGE];
    __shared__ __attribute__((aligned(16))) double sv[LB_STAGE][TS];
    __shared__ double red[RED][LB_LANES][LB_TF];
    const int fl = threadIdx.x % LB_TF, lane = threadIdx.x / LB_TF;
    const int64_t blk = (int64_t)blockIdx.x / ftiles, tile = (int64_t)blockIdx.x - blk * ftiles;
    const int64_t k = tile * LB_TF + fl, j0 = blk * TS;                     // the block's first resample within the chunk
    const double fv = k < Nf ? f[k] : 0.0;
    const int64_t n0 = (int64_t)blockIdx.y * slab_samples, n1 = n0 + slab_samples < N ? n0 + slab_samples : N;
    // staging: thread -> sample pair pp of the stage and the resamples h0 .. h0 + HALF - 1 of the block
    const int pp = threadIdx.x % (LB_STAGE / 2), h0 = (threadIdx.x / (LB_STAGE / 2)) * HALF;
    double m[HALF];
#pragma unroll
    for (int q = 0; q < HALF; ++q) m[q] = mean && j0 + h0 + q < count ? mean[r0 + j0 + h0 + q] : 0.0;
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    for (int64_t base = n0; base < n1; base += LB_STAGE) {
        const int cnt = (int)(n1 - base < LB_STAGE ? n1 - base : LB_STAGE);
        __syncthreads();                                                   // the previous stage has been walked
        if ((int)threadIdx.x < cnt) st[threadIdx.x] = t[base + threadIdx.x];
        const int64_t na = base + 2 * pp;                                  // (base is even: the pair of samples na, na + 1 is pair na >> 1)
        if (na < n1) {
            const bool two = na + 1 < n1;
            const double wa = w[na], wb = two ? w[na + 1] : 0.0;
#pragma unroll
            for (int q = 0; q < HALF; ++q) {
                double va = 0.0, vb = 0.0;
                if (j0 + h0 + q < count) {
                    uint64_t i0, i1;
                    boot_index_pair(seed, (uint64_t)(row0 + r0 + j0 + h0 + q), (uint64_t)(na >> 1), (uint64_t)N, &i0, &i1);
                    va = wa * (y[i0] - m[q]);
                    if (two) vb = wb * (y[i1] - m[q]);                     // (i1 < N whatever N is; the value is not used past the record)
                }
                sv[2 * pp][h0 + q] = va;
                sv[2 * pp + 1][h0 + q] = vb;
            }
        }
        __syncthreads();
        for (int i = lane; i < cnt; i += LB_LANES) {
            double sn, cs;
            lomb_sincos(fv, st[i], &sn, &cs);
            double v[TS];
#pragma unroll
            for (int q = 0; q < TS; ++q) v[q] = sv[i][q];
#pragma unroll
            for (int q = 0; q < TS; ++q) {
                acc[2 * q] = fma(v[q], cs, acc[2 * q]);
                acc[2 * q + 1] = fma(v[q], sn, acc[2 * q + 1]);
            }
        }
    }
    double *o = part + ((int64_t)blockIdx.y * 2 * count + 2 * j0) * Nf + k;
#pragma unroll
    for (int g = 0; g < NA / RED; ++g) {
        __syncthreads();                                                   // the previous round has been read
#pragma unroll
        for (int a = 0; a < RED; ++a) red[a][lane][fl] = acc[g * RED + a];
        __syncthreads();
        if (lane == 0 && k < Nf) {
#pragma unroll
            for (int a = 0; a < RED; ++a) {
                const int row = g * RED + a;                               // 2 q + {0, 1}
                if (j0 + row / 2 < count) o[(int64_t)row * Nf] = lomb_lane_sum(red[a], fl);
            }
        }
    }
}

// sums[e] = lomb_pairwise over the slabs of part[slab][e], e < count
__global__ void __launch_bounds__(256) lomb_boot_slab_sum_kernel(const double *__restrict__ part, int64_t nslab, int64_t count, double *__restrict__ sums) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    sums[e] = lomb_pairwise(part + e, count, nslab);
}

// ---- epilogue + maximum: workgroup = one resample of the chunk -------------------------------------------------------------------------------
// shared[{0, 1, 2, 3} Nf + k] = C, S, C2, S2 of the observed record; sums[(2 j + {0, 1}) Nf + k] = YC, YS of the chunk's resample j;
// mean, mom, maxv, maxi: per resample counted from row0 (r0: the chunk's first); power: Nf x B or nullptr; ndeg (+= the degenerate
// frequencies, by the first workgroup when count_deg: they are those of the observed record, the same for every resample)
__global__ void __launch_bounds__(256)
lomb_boot_epilogue_kernel(const double *__restrict__ shared, const double *__restrict__ sums, int64_t Nf, int64_t r0, const double *__restrict__ mean,
                          const double *__restrict__ mom, int fit_mean, int center, int psd, double Nsamples, double *__restrict__ power, double *__restrict__ maxv,
                          int64_t *__restrict__ maxi, int count_deg, int *__restrict__ ndeg) {
    __shared__ double rv[256];
    __shared__ int64_t ri[256];
    const int64_t j = blockIdx.x, r = r0 + j;
    const double Y = mom[4 * r], YY = mom[4 * r + 1], R = mom[4 * r + 2], removed = center ? mean[r] : 0.0;
    const double *yc = sums + (2 * j) * Nf, *ys = yc + Nf;
    double best = -1.0 / 0.0;
    int64_t at = Nf;
    int deg = 0;
    for (int64_t k = threadIdx.x; k < Nf; k += 256) {
        const LombFit ft = lomb_fit(shared[k], shared[Nf + k], shared[2 * Nf + k], shared[3 * Nf + k], yc[k], ys[k], Y, YY, R, removed, fit_mean, center, psd, Nsamples);
        if (ft.degenerate) ++deg;
        if (power) power[r * Nf + k] = ft.pw;
        if (ft.pw > best || at == Nf) { best = ft.pw; at = k; }          // ascending k: the first of equal values stays
    }
    if (count_deg && j == 0 && deg) atomicAdd(ndeg, deg);
    rv[threadIdx.x] = best; ri[threadIdx.x] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = rv[threadIdx.x], b = rv[threadIdx.x + s];
            const int64_t ia = ri[threadIdx.x], ib = ri[threadIdx.x + s];
            // a thread that saw no frequency holds index Nf and loses; ties go to the lower index
            const bool take = ib < Nf && (ia == Nf || b > a || (b == a && ib < ia));
            if (take) { rv[threadIdx.x] = b; ri[threadIdx.x] = ib; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { maxv[r] = rv[0]; maxi[r] = ri[0]; }
}

}  // namespace

// mean[B], mom[4 B] of the resamples row0 .. row0 + B - 1 (w: the normalised weights of the record)
int32_t launch_lomb_boot_moments(const double *y, const double *w, int64_t N, int64_t seed, int64_t row0, int64_t B, bool center, double *mean, double *mom,
                                 hipStream_t s) {
    hipLaunchKernelGGL(lomb_boot_moments_kernel, dim3((unsigned)B), dim3(256), 0, s, y, w, N, (uint64_t)seed, row0, center ? 1 : 0, mean, mom);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// sums[2 count][Nf] of the chunk's resamples r0 .. r0 + count - 1 (counted from row0); part: plan.nslab * 2 count * Nf doubles
int32_t launch_lomb_boot_sums(const double *t, const double *w, const double *y, int64_t N, int64_t seed, int64_t row0, int64_t r0, int64_t count,
                              const double *mean_or_null, const double *f_dev, int64_t Nf, const LombBootPlan &plan, double *part, double *sums, hipStream_t s) {
    const int64_t blocks = ceil_div(count, (int64_t)plan.ts);
    const dim3 grid((unsigned)(plan.ftiles * blocks), (unsigned)plan.nslab);
    if (plan.ts == 8)
        hipLaunchKernelGGL(lomb_boot_kernel<8>, grid, dim3(256), 0, s, t, w, y, N, (uint64_t)seed, row0, r0, count, mean_or_null, f_dev, Nf, plan.ftiles,
                           plan.slab_samples, part);
    else
        hipLaunchKernelGGL(lomb_boot_kernel<16>, grid, dim3(256), 0, s, t, w, y, N, (uint64_t)seed, row0, r0, count, mean_or_null, f_dev, Nf, plan.ftiles,
                           plan.slab_samples, part);
    const int64_t total = 2 * count * Nf;
    hipLaunchKernelGGL(lomb_boot_slab_sum_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, part, plan.nslab, total, sums);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_lomb_boot_epilogue(const double *shared, const double *sums, int64_t Nf, int64_t r0, int64_t count, const double *mean, const double *mom,
                                  bool fit_mean, bool center, bool psd, int64_t N, double *power_or_null, double *maxv, int64_t *maxi, bool count_deg, int *ndeg_dev,
                                  hipStream_t s) {
    hipLaunchKernelGGL(lomb_boot_epilogue_kernel, dim3((unsigned)count), dim3(256), 0, s, shared, sums, Nf, r0, mean, mom, fit_mean ? 1 : 0, center ? 1 : 0,
                       psd ? 1 : 0, (double)N, power_or_null, maxv, maxi, count_deg ? 1 : 0, ndeg_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace lpvs
