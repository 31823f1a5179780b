// fold.hip -- the fold statistics of non-uniformly sampled signals: phase dispersion minimisation with covers (pdm; Stellingwerf, ApJ 224,
// 953, 1978), the analysis-of-variance periodogram (aov; Schwarzenberg-Czerny, MNRAS 241, 153, 1989: the same sums) and the conditional
// entropy (Graham et al., MNRAS 434, 2629, 2013).  Hand-written HIP, gfx950; the definitions: include/lpvspectral.h g10; the decisions,
// the orders of the sums and the error model: fold_plan.h; DESIGN.md 4.18.  The record is quantised by bls.hip's kernels.
//
// PDM: pdm_kernel<F, TS, UNIT>, one launch per pass of TS signals, one workgroup of 256 threads per F frequencies.
//   zero, stage, fold, prefix   as bls_kernel (bls.hip), over nfine = nbins covers fine bins
//   pool     a thread owns the coarse bins m = tid, tid + 256, ...: the covers fine bins from m on, wrapping, two LDS reads per row; it adds
//            (s s) / r of those with r > 0, per signal, in ascending order, and counts them; a tree over the wave, four wave sums through LDS
//   write    thread 0 forms explained and the flag of every signal of the pass, and the count of non-empty coarse bins
// CONDITIONAL ENTROPY: cent_minmax_kernel and cent_vbin_kernel leave ymin, ymax and a byte per (signal, sample); cent_kernel<F, TS>:
//   zero     F copies TS count histograms of nbins mbins cells in LDS
//   fold     the phase bin of (t, f) once per (sample, frequency), then one 32-bit LDS atomic per signal of the pass, into the copy of the wave
//   merge    the copies into the first, by integer additions
//   entropy  per (frequency, signal): the row sums, then a thread adds the terms of its cells tid, tid + 256, ...; the same tree
// No cooperative launch, no spin-wait, nothing crosses workgroups but the degenerate counter and the min / max cells (integer atomics).
#include "lpvs_internal.h"
#include "fold_plan.h"
#include "fold_device.h"

namespace lpvs {
namespace {

typedef unsigned long long u64;

// lane 0 of every wave: the sum of the wave's 64 values by the tree of fold_plan.h (lane l takes lane l + 32, then l + 16, ... 1)
__device__ inline double fold_wave_tree(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

template <int F, int TS, bool UNIT>
__global__ void __launch_bounds__(256) pdm_kernel(const PdmArgs A, int c0) {
    constexpr int NR = TS + (UNIT ? 0 : 1);                                // 64-bit rows per frequency: qy of the TS signals, then qw
    extern __shared__ u64 lds[];
    __shared__ double red_s[4][TS];
    __shared__ int red_m[4];
    const int nb = A.nfine, nc = A.covers, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ns = A.ns;
    const int64_t N = A.N, k0 = (int64_t)blockIdx.x * F;
    u64 *H = lds;                                                          // [F][NR][nb]
    unsigned int *HC = reinterpret_cast<unsigned int *>(lds + F * NR * nb);   // [F][nb]
    for (int i = tid; i < F * NR * nb; i += 256) H[i] = 0;
    for (int i = tid; i < F * nb; i += 256) HC[i] = 0;
    double fv[F];
#pragma unroll
    for (int j = 0; j < F; ++j) fv[j] = k0 + j < A.Nf ? A.f[k0 + j] : 0.0;
    const double dnb = (double)nb;
    __syncthreads();
    // ---- fold
    for (int64_t base = 0; base < N; base += 256) {
        const int64_t n = base + tid;
        if (n >= N) break;
        const double tv = A.t[n];
        u64 qw = 0, qy[TS];
        if (!UNIT) qw = (u64)A.qw[n];
#pragma unroll
        for (int c = 0; c < TS; ++c) qy[c] = c0 + c < ns ? (u64)A.qy[(int64_t)(c0 + c) * N + n] : 0;
#pragma unroll
        for (int j = 0; j < F; ++j) {
            if (k0 + j >= A.Nf) continue;
            const int bin = bls_bin(fv[j], tv, nb, dnb);
            atomicAdd(&HC[j * nb + bin], 1u);
            if (!UNIT) atomicAdd(&H[(j * NR + TS) * nb + bin], qw);
#pragma unroll
            for (int c = 0; c < TS; ++c)
                if (c0 + c < ns) atomicAdd(&H[(j * NR + c) * nb + bin], qy[c]);
        }
    }
    __syncthreads();
    // ---- the raw histograms, when asked for: hist[k][0] = the weights (the counts with unit weights), hist[k][1 + c] = signal c
    if (A.hist || A.hcount) {
        for (int j = 0; j < F && k0 + j < A.Nf; ++j) {
            for (int b = tid; b < nb; b += 256) {
                if (A.hcount && c0 == 0) A.hcount[(k0 + j) * nb + b] = (int32_t)HC[j * nb + b];
                if (!A.hist) continue;
                long long *o = A.hist + (k0 + j) * (int64_t)(1 + ns) * nb + b;
                if (c0 == 0) o[0] = UNIT ? (long long)HC[j * nb + b] : (long long)H[(j * NR + TS) * nb + b];
#pragma unroll
                for (int c = 0; c < TS; ++c)
                    if (c0 + c < ns) o[(int64_t)(1 + c0 + c) * nb] = (long long)H[(j * NR + c) * nb + b];
            }
        }
        __syncthreads();
    }
    // ---- prefix sums: a wave per row
    for (int row = wave; row < F * (NR + 1); row += 4) {
        if (row < F * NR) bls_prefix_row(reinterpret_cast<long long *>(H) + row * nb, nb, lane);
        else bls_prefix_row(HC + (row - F * NR) * nb, nb, lane);
    }
    __syncthreads();
    // ---- the pooled between-bin sum over every cover
    for (int j = 0; j < F && k0 + j < A.Nf; ++j) {
        const int64_t kf = k0 + j;
        const long long *IY = reinterpret_cast<const long long *>(H) + j * NR * nb, *IW = IY + TS * nb;
        const unsigned int *IC = HC + j * nb;
        const long long Rq = UNIT ? (long long)N : IW[nb - 1];
        const unsigned int Ctot = IC[nb - 1];
        long long Sq[TS];
        double acc[TS];
        int M = 0;
#pragma unroll
        for (int c = 0; c < TS; ++c) { Sq[c] = IY[c * nb + nb - 1]; acc[c] = 0.0; }
        for (int m = tid; m < nb; m += 256) {
            const long long rq = UNIT ? (long long)bls_box<unsigned int>(IC, nb, m, nc, m > 0 ? IC[m - 1] : 0u, Ctot)
                                      : bls_box<long long>(IW, nb, m, nc, m > 0 ? IW[m - 1] : 0, Rq);
            if (rq <= 0) continue;
            ++M;
            const double rd = (double)rq;
#pragma unroll
            for (int c = 0; c < TS; ++c) {
                const double sd = (double)bls_box<long long>(IY + c * nb, nb, m, nc, m > 0 ? IY[c * nb + m - 1] : 0, Sq[c]);
                acc[c] = acc[c] + (sd * sd) / rd;
            }
        }
#pragma unroll
        for (int c = 0; c < TS; ++c) acc[c] = fold_wave_tree(acc[c]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) M += __shfl_down(M, off, 64);
        __syncthreads();                                                   // (thread 0 has read red_* of the previous frequency)
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < TS; ++c) red_s[wave][c] = acc[c];
            red_m[wave] = M;
        }
        __syncthreads();
        if (tid != 0) continue;
        const int Mt = (red_m[0] + red_m[1]) + (red_m[2] + red_m[3]);
        if (c0 == 0) A.nonempty[kf] = Mt;
        const bool bins_ok = Mt > nc && (long long)nc * N > (long long)Mt;
#pragma unroll
        for (int c = 0; c < TS; ++c) {
            const int cg = c0 + c;
            if (cg >= ns) continue;
            const double tot = (red_s[0][c] + red_s[1][c]) + (red_s[2][c] + red_s[3][c]);
            const double Sd = (double)Sq[c];
            const double sb = tot / (double)nc - (Sd * Sd) / (double)Rq;
            const int shv = A.shy[ns + cg], shy = A.shy[cg];
            const double inf = 1.0 / 0.0;
            const double YY = shv != kBlsNoShift ? bls_yy(A.yyacc[2 * cg], A.yyacc[2 * cg + 1], shv, A.log2n) : A.amax[ns + cg] == 0 ? 0.0 : inf;
            const double noise = lomb_yy_noise((double)N, A.center != 0, false, A.mom[2 * ns + cg], YY);
            const double dpos = sb > 0.0 ? sb : 0.0;                       // (a NaN -- R = 0 -- gives 0 and M = 0 flags it)
            const double delta = UNIT ? scalbn(dpos * (double)N, -2 * shy) : scalbn(dpos, kBlsWeightShift - 2 * shy);
            const bool live = bins_ok && A.amax[cg] != 0 && YY > noise && YY < inf && delta < inf;
            if (!live) atomicAdd(A.ndeg, 1ull);
            const int64_t o = (int64_t)cg * A.Nf + kf;
            A.explained[o] = live ? fmin(1.0, delta / YY) : 0.0;
            A.degenerate[o] = live ? 0 : 1;
        }
    }
}

template <int F, int TS>
int32_t pdm_launch_unit(const PdmArgs &A, bool unit, int c0, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(A.Nf, F));
    if (unit) hipLaunchKernelGGL((pdm_kernel<F, TS, true>), grid, dim3(256), lds, s, A, c0);
    else hipLaunchKernelGGL((pdm_kernel<F, TS, false>), grid, dim3(256), lds, s, A, c0);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
template <int F>
int32_t pdm_launch_ts(const PdmArgs &A, int ts, bool unit, int c0, size_t lds, hipStream_t s) {
    switch (ts) {
    case 1: return pdm_launch_unit<F, 1>(A, unit, c0, lds, s);
    case 2: return pdm_launch_unit<F, 2>(A, unit, c0, lds, s);
    case 4: return pdm_launch_unit<F, 4>(A, unit, c0, lds, s);
    default: set_error("pdm: no kernel for %d signals per pass", ts); return LPVS_EUNSUPPORTED;
    }
}

// ---- conditional entropy ---------------------------------------------------------------------------------------------------------------------
// lim[c] = the smallest key of y[c][.], lim[ns + c] = the largest (fold_plan.h: fold_key; initialised by the launcher): a block minimum and
// maximum, then one integer atomic each -- exact and order-free
__global__ void __launch_bounds__(256) cent_minmax_kernel(const double *__restrict__ y, int64_t N, int ns, u64 *__restrict__ lim) {
    __shared__ u64 lo[256], hi[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const u64 k = n < N ? fold_key(y[(int64_t)c * N + n]) : 0;
    lo[threadIdx.x] = n < N ? k : ~0ull;
    hi[threadIdx.x] = k;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const u64 a = lo[threadIdx.x + s], b = hi[threadIdx.x + s];
            if (a < lo[threadIdx.x]) lo[threadIdx.x] = a;
            if (b > hi[threadIdx.x]) hi[threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMin(&lim[c], lo[0]);
        atomicMax(&lim[ns + c], hi[0]);
    }
}

// vbin[c][n] = the value bin of y[c][n] (fold_plan.h: cent_value_bin); ylim[c] = {ymin, ymax}; degenerate[c]: ymax - ymin is 0 or not finite
__global__ void __launch_bounds__(256) cent_vbin_kernel(const double *__restrict__ y, int64_t N, int ns, int mbins, const u64 *__restrict__ lim,
                                                        unsigned char *__restrict__ vbin, double *__restrict__ ylim, int32_t *__restrict__ degenerate) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const double ymin = fold_unkey(lim[c]), ymax = fold_unkey(lim[ns + c]), den = ymax - ymin;
    if (n < N) vbin[(int64_t)c * N + n] = (unsigned char)cent_value_bin(y[(int64_t)c * N + n], ymin, den, mbins);
    if (n == 0) {
        ylim[2 * c] = ymin;
        ylim[2 * c + 1] = ymax;
        degenerate[c] = (den > 0.0 && den < 1.0 / 0.0) ? 0 : 1;
    }
}

template <int F, int TS>
__global__ void __launch_bounds__(256) cent_kernel(const CentArgs A, int c0, int copies) {
    extern __shared__ unsigned int cnt[];                                  // [F][copies][TS][cells]
    __shared__ unsigned int rows[kCentMaxBins];
    __shared__ double red[4];
    const int nb = A.nbins, mb = A.mbins, cells = nb * mb, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ns = A.ns;
    const int64_t N = A.N, k0 = (int64_t)blockIdx.x * F;
    for (int i = tid; i < F * copies * TS * cells; i += 256) cnt[i] = 0;
    double fv[F];
#pragma unroll
    for (int j = 0; j < F; ++j) fv[j] = k0 + j < A.Nf ? A.f[k0 + j] : 0.0;
    const double dnb = (double)nb;
    const int copy = wave % copies;
    __syncthreads();
    // ---- fold
    for (int64_t base = 0; base < N; base += 256) {
        const int64_t n = base + tid;
        if (n >= N) break;
        const double tv = A.t[n];
        int vb[TS];
#pragma unroll
        for (int c = 0; c < TS; ++c) vb[c] = c0 + c < ns ? (int)A.vbin[(int64_t)(c0 + c) * N + n] : 0;
#pragma unroll
        for (int j = 0; j < F; ++j) {
            if (k0 + j >= A.Nf) continue;
            const int bin = bls_bin(fv[j], tv, nb, dnb);
            unsigned int *C = cnt + (j * copies + copy) * TS * cells + bin * mb;
#pragma unroll
            for (int c = 0; c < TS; ++c)
                if (c0 + c < ns) atomicAdd(&C[c * cells + vb[c]], 1u);
        }
    }
    __syncthreads();
    // ---- merge the copies into the first
    if (copies > 1) {
        for (int i = tid; i < F * TS * cells; i += 256) {
            const int j = i / (TS * cells), q = i - j * (TS * cells);
            unsigned int *C = cnt + j * copies * TS * cells + q;
            unsigned int sum = C[0];
            for (int v = 1; v < copies; ++v) sum += C[v * TS * cells];
            C[0] = sum;
        }
        __syncthreads();
    }
    // ---- the entropy of every (frequency, signal)
    for (int j = 0; j < F && k0 + j < A.Nf; ++j) {
        const int64_t kf = k0 + j;
        for (int c = 0; c < TS && c0 + c < ns; ++c) {
            const int cg = c0 + c;
            const unsigned int *C = cnt + (j * copies * TS + c) * cells;
            if (A.hist) {
                int32_t *o = A.hist + (kf * ns + cg) * (int64_t)cells;
                for (int q = tid; q < cells; q += 256) o[q] = (int32_t)C[q];
            }
            for (int i = tid; i < nb; i += 256) {
                unsigned int sum = 0;
                for (int v = 0; v < mb; ++v) sum += C[i * mb + v];
                rows[i] = sum;
            }
            __syncthreads();
            double acc = 0.0;
            for (int q = tid; q < cells; q += 256) {
                const unsigned int nij = C[q];
                if (nij == 0) continue;
                acc = acc + (double)nij * log((double)rows[q / mb] / (double)nij);
            }
            acc = fold_wave_tree(acc);
            if (lane == 0) red[wave] = acc;
            __syncthreads();
            if (tid == 0) A.entropy[(int64_t)cg * A.Nf + kf] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)N;
            __syncthreads();                                               // (rows and red are free again)
        }
    }
}

template <int F>
int32_t cent_launch_ts(const CentArgs &A, const CentPlan &plan, int c0, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(A.Nf, F));
    const size_t lds = (size_t)plan.lds_bytes;
    switch (plan.ts) {
    case 1: hipLaunchKernelGGL((cent_kernel<F, 1>), grid, dim3(256), lds, s, A, c0, plan.copies); break;
    case 2: hipLaunchKernelGGL((cent_kernel<F, 2>), grid, dim3(256), lds, s, A, c0, plan.copies); break;
    case 4: hipLaunchKernelGGL((cent_kernel<F, 4>), grid, dim3(256), lds, s, A, c0, plan.copies); break;
    default: set_error("conditional_entropy: no kernel for %d signals per pass", plan.ts); return LPVS_EUNSUPPORTED;
    }
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace

// one launch per pass of plan.ts signals; A.ndeg: zeroed here
int32_t launch_pdm(const PdmArgs &A, const PdmPlan &plan, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(A.ndeg, 0, sizeof(unsigned long long), s));
    const size_t lds = (size_t)plan.lds_bytes;
    for (int pass = 0; pass < plan.passes; ++pass) {
        const int c0 = pass * plan.ts;
        switch (plan.F) {
        case 1: LPVS_TRY(pdm_launch_ts<1>(A, plan.ts, plan.unit != 0, c0, lds, s)); break;
        case 2: LPVS_TRY(pdm_launch_ts<2>(A, plan.ts, plan.unit != 0, c0, lds, s)); break;
        case 4: LPVS_TRY(pdm_launch_ts<4>(A, plan.ts, plan.unit != 0, c0, lds, s)); break;
        default: set_error("pdm: no kernel for %d frequencies per workgroup", plan.F); return LPVS_EUNSUPPORTED;
        }
    }
    return LPVS_OK;
}

int32_t launch_cent_prepare(const double *y, int64_t N, int64_t ns, int mbins, unsigned long long *lim_dev, unsigned char *vbin, double *ylim_dev,
                            int32_t *degenerate_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(lim_dev, 0xff, sizeof(unsigned long long) * (size_t)ns, s));
    LPVS_HIP(hipMemsetAsync(lim_dev + ns, 0, sizeof(unsigned long long) * (size_t)ns, s));
    const dim3 grid((unsigned)ceil_div(N, 256), (unsigned)ns);
    hipLaunchKernelGGL(cent_minmax_kernel, grid, dim3(256), 0, s, y, N, (int)ns, lim_dev);
    LPVS_HIP(hipGetLastError());
    hipLaunchKernelGGL(cent_vbin_kernel, grid, dim3(256), 0, s, y, N, (int)ns, mbins, lim_dev, vbin, ylim_dev, degenerate_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t launch_cent(const CentArgs &A, const CentPlan &plan, hipStream_t s) {
    for (int pass = 0; pass < plan.passes; ++pass) {
        const int c0 = pass * plan.ts;
        switch (plan.F) {
        case 1: LPVS_TRY(cent_launch_ts<1>(A, plan, c0, s)); break;
        case 2: LPVS_TRY(cent_launch_ts<2>(A, plan, c0, s)); break;
        case 4: LPVS_TRY(cent_launch_ts<4>(A, plan, c0, s)); break;
        default: set_error("conditional_entropy: no kernel for %d frequencies per workgroup", plan.F); return LPVS_EUNSUPPORTED;
        }
    }
    return LPVS_OK;
}

}  // namespace lpvs
