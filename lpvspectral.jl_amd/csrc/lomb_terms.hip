// lomb_terms.hip -- the multi-harmonic Lomb-Scargle periodogram, lombscargle(..., nterms = K) (hand-written HIP, gfx950; the definition:
// include/lpvspectral.h g7; the decisions: lomb_terms_plan.h).
//
// Per frequency f_k, with normalised weights w and phases phi = 2 pi f_k t_n of the exact products:
//   C_m = sum w cos m phi, S_m = sum w sin m phi (m = 1 .. 2K),   YC_h = sum w y_c cos h phi, YS_h = sum w y_c sin h phi (h = 1 .. K, per signal)
// and the weighted least-squares fit of y ~ c + sum_h a_h cos h phi + b_h sin h phi from the 2K x 2K normal equations these sums form.
//
// SUMS: lomb_terms_kernel<K, TS>.  A workgroup = 64 frequencies x 4 sample lanes walks one slab of samples, staged through LDS 256 at a
// time, exactly as lomb_direct_kernel does.  Per (sample, frequency) ONE sincospi (lomb_sincos: the phase of the exact product) gives
// z_1 = cos phi + i sin phi, and the harmonics 2 .. 2K follow by complex rotation z_m = z_{m-1} z_1, written with explicit fma.  The
// 4K + 2K TS accumulators live in registers: every loop over them has constant bounds (K and TS are template parameters) and is unrolled,
// so no index is formed at run time.  The four lanes are added as (0 + 1) + (2 + 3) through LDS four accumulators at a time (8 KB, not
// one array of all of them), the slabs by lomb_slab_sum_kernel's pairwise tree: a fixed order, so two calls give the same bits and a
// signal's sums do not depend on which other signals ride along.
//
// EPILOGUE: lomb_terms_epilogue_kernel<K>, one thread per (frequency, signal): A, g, b from the sums, the floating-mean terms, A = L D L^T
// without pivoting (the lower triangle in registers, static indices), the solve, the constant-signal rule of g4, power and coefficients.
//
// Only direct sums: every harmonic of a progression of frequencies is a progression too and could take the transforms of nufft.hip, 2K
// families instead of g4's two -- not built.
#include "lpvs_internal.h"
#include "lomb_terms_plan.h"
#include "lomb_device.h"

namespace lpvs {
namespace {

// accumulators of a thread: [2 (m - 1) + {0, 1}] = C_m, S_m, m = 1 .. 2K; [4K + 2K c + 2 (h - 1) + {0, 1}] = YC_h, YS_h of the thread's signal c
template <int K, int TS>
__device__ inline void lomb_terms_walk_stage(double fv, const double *st, const double *sw, const double (*swy)[LB_STAGE], int cnt, int lane, double *acc) {
    for (int i = lane; i < cnt; i += LB_LANES) {
        double s1, c1;
        lomb_sincos(fv, st[i], &s1, &c1);
        const double wv = sw[i];
        double v[TS];
#pragma unroll
        for (int c = 0; c < TS; ++c) v[c] = swy[c][i];
        double cm = c1, sm = s1;
#pragma unroll
        for (int m = 1; m <= 2 * K; ++m) {
            if (m > 1) {                                                   // z_m = z_{m-1} z_1
                const double cn = fma(cm, c1, -(sm * s1)), sn = fma(sm, c1, cm * s1);
                cm = cn; sm = sn;
            }
            acc[2 * (m - 1)] = fma(wv, cm, acc[2 * (m - 1)]);
            acc[2 * (m - 1) + 1] = fma(wv, sm, acc[2 * (m - 1) + 1]);
            if (m <= K) {
#pragma unroll
                for (int c = 0; c < TS; ++c) {
                    acc[4 * K + 2 * K * c + 2 * (m - 1)] = fma(v[c], cm, acc[4 * K + 2 * K * c + 2 * (m - 1)]);
                    acc[4 * K + 2 * K * c + 2 * (m - 1) + 1] = fma(v[c], sm, acc[4 * K + 2 * K * c + 2 * (m - 1) + 1]);
                }
            }
        }
    }
}

// ---- sums: workgroup (tile of 64 frequencies, slab of samples, block of TS signals) ----------------------------------------------------
// part[(slab nrow + row) Nf + k], nrow = 4K + 2K ns: rows C_m, S_m (written by signal block 0), then YC_h, YS_h of every signal
template <int K, int TS>
__global__ void __launch_bounds__(256)
lomb_terms_kernel(const double *__restrict__ t, const double *__restrict__ w, const double *__restrict__ wy, int64_t N, int ns, const double *__restrict__ f,
                  int64_t Nf, int64_t slab_samples, double *__restrict__ part) {
    constexpr int NA = 4 * K + 2 * K * TS;
    static_assert(K >= 1 && K <= kLombMaxTerms && NA <= kLombTermsMaxAcc, "the accumulators of a thread");
    __shared__ double st[LB_STAGE], sw[LB_STAGE], swy[TS][LB_STAGE];
    __shared__ double red[LB_LANES][LB_LANES][LB_TF];                      // [accumulator of the group][sample lane][frequency]
    const int fl = threadIdx.x % LB_TF, lane = threadIdx.x / LB_TF;
    const int64_t k = (int64_t)blockIdx.x * LB_TF + fl;
    const int c0 = blockIdx.z * TS;
    const double fv = k < Nf ? f[k] : 0.0;
    const int64_t n0 = (int64_t)blockIdx.y * slab_samples, n1 = n0 + slab_samples < N ? n0 + slab_samples : N;
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    for (int64_t base = n0; base < n1; base += LB_STAGE) {
        const int cnt = (int)(n1 - base < LB_STAGE ? n1 - base : LB_STAGE);
        __syncthreads();                                                   // the previous stage has been walked
        if ((int)threadIdx.x < cnt) {
            const int64_t n = base + threadIdx.x;
            st[threadIdx.x] = t[n];
            sw[threadIdx.x] = w[n];
#pragma unroll
            for (int c = 0; c < TS; ++c) swy[c][threadIdx.x] = c0 + c < ns ? wy[(int64_t)(c0 + c) * N + n] : 0.0;
        }
        __syncthreads();
        lomb_terms_walk_stage<K, TS>(fv, st, sw, swy, cnt, lane, acc);
    }
    // the lanes, four accumulators at a time: the thread of lane l adds the four lanes of accumulator a0 + l and files it
    const int nrow = 4 * K + 2 * K * ns;
    double *o = part + (int64_t)blockIdx.y * nrow * Nf + k;
#pragma unroll
    for (int a0 = 0; a0 < NA; a0 += LB_LANES) {
        __syncthreads();                                                   // the previous group has been read
#pragma unroll
        for (int j = 0; j < LB_LANES; ++j)
            if (a0 + j < NA) red[j][lane][fl] = acc[a0 + j];
        __syncthreads();
        const int a = a0 + lane;
        if (a < NA && k < Nf) {
            const double v = lomb_lane_sum(red[lane], fl);
            if (a < 4 * K) { if (blockIdx.z == 0) o[(int64_t)a * Nf] = v; }
            else {
                const int c = c0 + (a - 4 * K) / (2 * K), r = (a - 4 * K) % (2 * K);
                if (c < ns) o[(int64_t)(4 * K + 2 * K * c + r) * Nf] = v;
            }
        }
    }
}

// ---- epilogue: one thread per (frequency, signal) ----------------------------------------------------------------------------------------
// The unknowns are ordered (a_1, b_1, a_2, b_2, ...): index 2 (h - 1) + p, p = 0 the cosine and 1 the sine of harmonic h.
// mom[2 c + {0, 1}] = Y_c, YY_c of the (centred) signal, mom[2 ns + c] = sum w y_c^2 of the signal as given; mean[c]: its weighted mean.
// coef: 2K + 1 planes of Nf x ns: a_h, b_h (h = 1 .. K), then c.
constexpr int lomb_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // the lower triangle by rows, j <= i
template <int K>
__global__ void __launch_bounds__(kLombTermsEpilogueBlock)
lomb_terms_epilogue_kernel(const double *__restrict__ sums, int64_t Nf, int ns, const double *__restrict__ mom, const double *__restrict__ mean, int fit_mean,
                           int center, int psd, double Nsamples, double *__restrict__ power, double *__restrict__ coef, int *__restrict__ ndegenerate) {
    constexpr int n = 2 * K;
    const int64_t k = (int64_t)blockIdx.x * kLombTermsEpilogueBlock + threadIdx.x;
    const int c = blockIdx.y;
    if (k >= Nf) return;
    // g = (C_1, S_1, ..., C_K, S_K) and the sums of the harmonics 0 .. 2K
    double Cm[2 * K + 1], Sm[2 * K + 1], g[n], b[n];
    Cm[0] = 1.0; Sm[0] = 0.0;
#pragma unroll
    for (int m = 1; m <= 2 * K; ++m) {
        Cm[m] = sums[(int64_t)(2 * (m - 1)) * Nf + k];
        Sm[m] = sums[(int64_t)(2 * (m - 1) + 1) * Nf + k];
    }
    const double *sy = sums + (int64_t)(4 * K + 2 * K * c) * Nf + k;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        g[i] = i % 2 == 0 ? Cm[i / 2 + 1] : Sm[i / 2 + 1];
        b[i] = sy[(int64_t)i * Nf];
    }
    const double Y = mom[2 * c], YY0 = mom[2 * c + 1], removed = center ? mean[c] : 0.0;
    const double yy_noise = lomb_yy_noise(Nsamples, center != 0, fit_mean != 0, mom[2 * ns + c], YY0);
    const double YY = fit_mean ? fma(-Y, Y, YY0) : YY0;
    // A (lower triangle): cos h cos j = (C_{h-j} + C_{h+j}) / 2, sin h sin j = (C_{h-j} - C_{h+j}) / 2,
    // sin h cos j = (S_{h+j} + S_{h-j}) / 2, cos h sin j = (S_{h+j} - S_{h-j}) / 2 for h >= j; then A -= g g^T, b -= Y g (fit_mean)
    double A[n * (n + 1) / 2];
#pragma unroll
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const int h = i / 2 + 1, q = j / 2 + 1, pi = i % 2, pj = j % 2;
            double v;
            if (pi == pj) v = pi == 0 ? 0.5 * (Cm[h - q] + Cm[h + q]) : 0.5 * (Cm[h - q] - Cm[h + q]);
            else v = pi == 1 ? 0.5 * (Sm[h + q] + Sm[h - q]) : 0.5 * (Sm[h + q] - Sm[h - q]);
            A[lomb_tri(i, j)] = fit_mean ? fma(-g[i], g[j], v) : v;
        }
    }
    if (fit_mean) {
#pragma unroll
        for (int i = 0; i < n; ++i) b[i] = fma(-Y, g[i], b[i]);
    }
    // A = L D L^T in place, row by row, no pivoting: L below the diagonal, the pivots d_j on it.  A pivot that fails
    // d_j > kLombDegenerate marks the frequency (and is replaced by 1 so that what follows stays finite; nothing of it is returned).
    bool degenerate = false;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        double d = A[lomb_tri(j, j)];
#pragma unroll
        for (int q = 0; q < j; ++q) d = fma(-(A[lomb_tri(j, q)] * A[lomb_tri(j, q)]), A[lomb_tri(q, q)], d);
        if (!(d > kLombDegenerate)) { degenerate = true; d = 1.0; }
        A[lomb_tri(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < n; ++i) {
            double v = A[lomb_tri(i, j)];
#pragma unroll
            for (int q = 0; q < j; ++q) v = fma(-(A[lomb_tri(i, q)] * A[lomb_tri(q, q)]), A[lomb_tri(j, q)], v);
            A[lomb_tri(i, j)] = v / d;
        }
    }
    // L z = b, z /= d, L^T theta = z
    double th[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
        double v = b[i];
#pragma unroll
        for (int q = 0; q < i; ++q) v = fma(-A[lomb_tri(i, q)], th[q], v);
        th[i] = v;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) th[i] = th[i] / A[lomb_tri(i, i)];
#pragma unroll
    for (int i = n - 1; i >= 0; --i) {
        double v = th[i];
#pragma unroll
        for (int q = i + 1; q < n; ++q) v = fma(-A[lomb_tri(q, i)], th[q], v);
        th[i] = v;
    }
    double p = 0.0, cst = Y;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        p = fma(b[i], th[i], p);
        cst = fma(-g[i], th[i], cst);
    }
    if (degenerate && c == 0) atomicAdd(ndegenerate, 1);
    const double pw = psd ? p * (0.5 * Nsamples) : (YY > yy_noise ? p / YY : 0.0);
    const int64_t e = (int64_t)c * Nf + k, plane = Nf * ns;
    power[e] = degenerate ? 0.0 : pw;
    if (coef) {
#pragma unroll
        for (int i = 0; i < n; ++i) coef[(int64_t)i * plane + e] = degenerate ? 0.0 : th[i];
        coef[(int64_t)n * plane + e] = degenerate ? 0.0 : removed + (fit_mean ? cst : 0.0);
    }
}

template <int K>
void lomb_terms_launch_k(const double *t, const double *w, const double *wy, int64_t N, int64_t ns, const double *f_dev, int64_t Nf, const LombTermsPlan &pl,
                         double *part, hipStream_t s) {
    const dim3 grid((unsigned)pl.ftiles, (unsigned)pl.nslab, (unsigned)pl.sblocks);
    constexpr int TSM = 4 * K + 2 * K * 4 <= kLombTermsMaxAcc ? 4 : 2;    // the block of signals of a multi-signal call (lomb_terms_ts)
    if (pl.ts == 1) hipLaunchKernelGGL((lomb_terms_kernel<K, 1>), grid, dim3(256), 0, s, t, w, wy, N, (int)ns, f_dev, Nf, pl.slab_samples, part);
    else hipLaunchKernelGGL((lomb_terms_kernel<K, TSM>), grid, dim3(256), 0, s, t, w, wy, N, (int)ns, f_dev, Nf, pl.slab_samples, part);
}
template <int K>
void lomb_terms_epilogue_k(const double *sums, int64_t Nf, int64_t ns, const double *mom_dev, const double *mean_dev, bool fit_mean, bool center, bool psd, int64_t N,
                           double *power, double *coef, int *ndeg_dev, hipStream_t s) {
    hipLaunchKernelGGL(lomb_terms_epilogue_kernel<K>, dim3((unsigned)ceil_div(Nf, kLombTermsEpilogueBlock), (unsigned)ns), dim3(kLombTermsEpilogueBlock), 0, s, sums,
                       Nf, (int)ns, mom_dev, mean_dev, fit_mean ? 1 : 0, center ? 1 : 0, psd ? 1 : 0, (double)N, power, coef, ndeg_dev);
}

}  // namespace

// sums[(4K + 2K ns)][Nf] by direct summation; part: pl.part_doubles doubles.  w, wy: launch_lomb_moments' (lomb.hip)
int32_t launch_lomb_terms_sums(const double *t, const double *w, const double *wy, int64_t N, int64_t ns, const double *f_dev, int64_t Nf, const LombTermsPlan &pl,
                               double *part, double *sums, hipStream_t s) {
    if (pl.status != kLombTermsOk || pl.ts != lomb_terms_ts(pl.K, ns)) { set_error("lombscargle: a plan that was refused reached the kernels"); return LPVS_EARGUMENT; }
    switch (pl.K) {
        case 1: lomb_terms_launch_k<1>(t, w, wy, N, ns, f_dev, Nf, pl, part, s); break;
        case 2: lomb_terms_launch_k<2>(t, w, wy, N, ns, f_dev, Nf, pl, part, s); break;
        case 3: lomb_terms_launch_k<3>(t, w, wy, N, ns, f_dev, Nf, pl, part, s); break;
        case 4: lomb_terms_launch_k<4>(t, w, wy, N, ns, f_dev, Nf, pl, part, s); break;
        case 5: lomb_terms_launch_k<5>(t, w, wy, N, ns, f_dev, Nf, pl, part, s); break;
        case 6: lomb_terms_launch_k<6>(t, w, wy, N, ns, f_dev, Nf, pl, part, s); break;
        default: set_error("lombscargle: nterms = %d has no kernel", pl.K); return LPVS_EARGUMENT;
    }
    LPVS_HIP(hipGetLastError());
    return launch_lomb_slab_sum(part, pl.nslab, pl.rows * Nf, sums, s);
}
// power[ns][Nf] (column-major Nf x ns), coef[2K + 1][ns][Nf] or nullptr; ndeg_dev: one int, zeroed here
int32_t launch_lomb_terms_epilogue(int K, const double *sums, int64_t Nf, int64_t ns, const double *mom_dev, const double *mean_dev, bool fit_mean, bool center,
                                   bool psd, int64_t N, double *power, double *coef, int *ndeg_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(ndeg_dev, 0, sizeof(int), s));
    switch (K) {
        case 1: lomb_terms_epilogue_k<1>(sums, Nf, ns, mom_dev, mean_dev, fit_mean, center, psd, N, power, coef, ndeg_dev, s); break;
        case 2: lomb_terms_epilogue_k<2>(sums, Nf, ns, mom_dev, mean_dev, fit_mean, center, psd, N, power, coef, ndeg_dev, s); break;
        case 3: lomb_terms_epilogue_k<3>(sums, Nf, ns, mom_dev, mean_dev, fit_mean, center, psd, N, power, coef, ndeg_dev, s); break;
        case 4: lomb_terms_epilogue_k<4>(sums, Nf, ns, mom_dev, mean_dev, fit_mean, center, psd, N, power, coef, ndeg_dev, s); break;
        case 5: lomb_terms_epilogue_k<5>(sums, Nf, ns, mom_dev, mean_dev, fit_mean, center, psd, N, power, coef, ndeg_dev, s); break;
        case 6: lomb_terms_epilogue_k<6>(sums, Nf, ns, mom_dev, mean_dev, fit_mean, center, psd, N, power, coef, ndeg_dev, s); break;
        default: set_error("lombscargle: nterms = %d has no kernel", K); return LPVS_EARGUMENT;
    }
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace lpvs
