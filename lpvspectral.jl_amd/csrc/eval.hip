// eval.hip -- evaluating a fitted model at samples (predict / residual / fva; hand-written HIP, gfx950).
//
//   yhat_m[c] = s sum_f sum_j K_j(v_m) Re( p[f + j Nf, c] exp(i phi_fm) ),   phi_fm = w_f x_m
//
// for both families: LPV (s = 1, K the activations of basis.hip, p = SpectralExt.x) and Fourier (s = 1 / sqrt(2 Nf), one basis function
// K = 1, w_f = fl(2 pi f_f), p = what ls_spectral returns).  It is the regressor times the coefficients without the N x n regressor.
//
// DIRECT path (any frequency grid): a thread owns a sample, loops over the frequencies with one sincos each -- the phase is the ROUNDED
// product fl(w_f x_m), as basis.hip forms it -- and keeps (basis function, column) accumulators in registers (eval_plan.h: eval_tiling);
// the coefficients pass through LDS in chunks of frequencies.
//
// TYPE-2 NON-UNIFORM FFT (w_f = a + f D + eps_f, admitted by eval_plan.h: eval_admit): the adjoint of nufft.hip's three steps,
//   1. coefficients / phihat(f) (host, from nufft.hip's long-double quadrature),
//   2. grid synthesis  g[k] = sum_f q_f e^{2 pi i f k / nf},  k < nf: a pruned direct DFT with the trig from an exact table indexed by
//      f k mod nf (Nf nf complex MACs per grid: 1e6 at cfg3's shape, not worth an FFT),
//   3. interpolation: a thread owns a sample, takes its cell and 16 kernel values from nufft_coord.h and reads 16 consecutive grid values
//      (periodic wrap) per grid; a rotation by e^{i a x_m} (phase reduced in double-double) serves a progression that does not start at
//      0, and when some eps_f != 0 a twin grid with coefficients i eps_f p_f, multiplied by x_m, adds the first-order term as the
//      structured Gram does.
// It is a gather: no atomics, the same bits every time.  The phase is that of the REAL product w x, half an ulp of phase away from the
// direct path's (DESIGN 6.2's 4.5e-16 max|w| max|x|).
//
// RESIDUAL EPILOGUE (both paths): with y the output is e = y - yhat; every workgroup leaves one partial of sum(e) and sum(e^2) per column
// (a pairwise tree over its 256 samples), and eval_sums_kernel adds the slabs in a fixed order -- no floating-point atomics.
// A column of a multi-column call goes through exactly the operations of a single-column call: the same bits.
#include "lpvs_internal.h"
#include "basis_device.h"
#include "nufft_coord.h"

namespace lpvs {
namespace {

constexpr int EV_TJ = kEvalBasisTile, EV_FC = kEvalFreqChunk;

// the normalising sum of a sample's activations: sequential, as basis_table_kernel adds it
__device__ inline double eval_basis_sum(double v, const EvalBasis &B) {
    double sum = 0;
    for (int j = 0; j < B.nb; ++j) {
        const double k = basis_activation(v, B.vc[j], B.gamma, B.coulomb);
        sum = j == 0 ? k : sum + k;
    }
    return sum;
}
// K_j(v); ksum: eval_basis_sum (read with normalize only).  vc == nullptr: the Fourier family's single K = 1
__device__ inline double eval_basis_value(double v, const EvalBasis &B, int j, double ksum) {
    if (!B.vc) return 1.0;
    const double k = basis_activation(v, B.vc[j], B.gamma, B.coulomb);
    return B.normalize ? k / ksum : k;                                      // src/lsfft.jl:199
}

// sum over the workgroup's 256 threads in a pairwise tree (every thread calls it)
__device__ inline double eval_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// output and partial sums of one column: o = s yhat, or y - s yhat.  part[(2 c + {0, 1}) nslab + workgroup] = sum o, sum o^2
__device__ inline void eval_store(double yh, double scale, const double *__restrict__ y, int64_t m, bool valid, int64_t M, int c, double *__restrict__ out,
                                  double *__restrict__ part, int64_t nslab, double *red) {
    double o = scale * yh;
    if (y && valid) o = y[m] - o;
    if (valid) out[(int64_t)c * M + m] = o;
    if (part) {                                                             // (uniform)
        const double s1 = eval_block_sum(valid ? o : 0.0, red), s2 = eval_block_sum(valid ? o * o : 0.0, red);
        if (threadIdx.x == 0) {
            part[(int64_t)(2 * c) * nslab + blockIdx.x] = s1;
            part[(int64_t)(2 * c + 1) * nslab + blockIdx.x] = s2;
        }
    }
}

// ---- direct path: workgroup (256 samples, block of TC columns) -------------------------------------------------------------------------
// P[(c nb + j) Nf + f] = p[f + j Nf, c] as (re, im)
template <int TC>
__global__ void __launch_bounds__(256)
eval_direct_kernel(const double *__restrict__ x, const double *__restrict__ v, const double *__restrict__ y, int64_t M, const double *__restrict__ w, int Nf,
                   const double2 *__restrict__ P, int nc, EvalBasis B, double scale, double *__restrict__ out, double *__restrict__ part, int64_t nslab) {
    __shared__ double2 sP[EV_FC][EV_TJ][TC];
    __shared__ double sw[EV_FC];
    __shared__ double red[256];
    const int64_t m = (int64_t)blockIdx.x * kEvalBlock + threadIdx.x;
    const bool valid = m < M;
    const int c0 = blockIdx.y * TC, nb = B.nb;
    const double xv = valid ? x[m] : 0.0, vv = valid && B.vc ? v[m] : 0.0;
    const double ksum = B.vc && B.normalize ? eval_basis_sum(vv, B) : 1.0;
    double yh[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) yh[c] = 0.0;
    for (int j0 = 0; j0 < nb; j0 += EV_TJ) {                               // passes over the frequencies: eval_tiling's jpasses
        const int jn = nb - j0 < EV_TJ ? nb - j0 : EV_TJ;
        double acc[EV_TJ][TC];
#pragma unroll
        for (int j = 0; j < EV_TJ; ++j)
#pragma unroll
            for (int c = 0; c < TC; ++c) acc[j][c] = 0.0;
        for (int f0 = 0; f0 < Nf; f0 += EV_FC) {
            const int fn = Nf - f0 < EV_FC ? Nf - f0 : EV_FC;
            __syncthreads();                                               // the previous chunk has been read
            for (int e = threadIdx.x; e < EV_FC * EV_TJ * TC; e += 256) {
                const int c = e % TC, j = (e / TC) % EV_TJ, fl = e / (TC * EV_TJ);
                double2 pv = make_double2(0.0, 0.0);
                if (fl < fn && j < jn && c0 + c < nc) pv = P[((int64_t)(c0 + c) * nb + j0 + j) * Nf + f0 + fl];
                sP[fl][j][c] = pv;
            }
            if (threadIdx.x < EV_FC) sw[threadIdx.x] = (int)threadIdx.x < fn ? w[f0 + threadIdx.x] : 0.0;
            __syncthreads();
            for (int fl = 0; fl < fn; ++fl) {
                const double phi = sw[fl] * xv;                            // rounded, as trig_table_kernel / fourier_regressor_colmajor_kernel
                double sn, cs;
                sincos(phi, &sn, &cs);
#pragma unroll
                for (int j = 0; j < EV_TJ; ++j) {
                    if (j >= jn) break;                                    // (uniform)
#pragma unroll
                    for (int c = 0; c < TC; ++c) {
                        // Re(p e^{i phi}) = re cos - im sin is formed first and added as ONE term: the chain behind an accumulator is
                        // Nf additions long, not 2 Nf (the bound of tests/_eval_ref.py counts them)
                        const double2 pv = sP[fl][j][c];
                        acc[j][c] = acc[j][c] + fma(pv.x, cs, -(pv.y * sn));
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < EV_TJ; ++j) {
            if (j >= jn) break;
            const double kj = eval_basis_value(vv, B, j0 + j, ksum);
#pragma unroll
            for (int c = 0; c < TC; ++c) yh[c] = fma(kj, acc[j][c], yh[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < TC; ++c)
        if (c0 + c < nc) eval_store(yh[c], scale, y, m, valid, M, c0 + c, out, part, nslab, red);   // (uniform)
}

// ---- type 2, step 2: the fine grids ----------------------------------------------------------------------------------------------------
// tw[m] = e^{2 pi i m / nf}, exact arguments (nf is a power of two)
__global__ void __launch_bounds__(256) eval_twiddle_kernel(int nf, double2 *__restrict__ tw) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= nf) return;
    double sn, cs;
    sincospi(2.0 * (double)m / (double)nf, &sn, &cs);
    tw[m] = make_double2(cs, sn);
}
// grid[g][k] = sum_f Q[g][f] e^{2 pi i f k / nf}: workgroup (256 grid points, grid g), thread = grid point; f k < 2^26
__global__ void __launch_bounds__(256)
eval_grid_kernel(const double2 *__restrict__ Q, int Nf, int nf, const double2 *__restrict__ tw, double2 *__restrict__ grid) {
    __shared__ double2 sq[256];
    const int g = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x, mask = nf - 1;   // nf is a multiple of 256
    double gr = 0.0, gi = 0.0;
    for (int f0 = 0; f0 < Nf; f0 += 256) {
        const int fn = Nf - f0 < 256 ? Nf - f0 : 256;
        __syncthreads();
        if ((int)threadIdx.x < fn) sq[threadIdx.x] = Q[(int64_t)g * Nf + f0 + threadIdx.x];
        __syncthreads();
        for (int fl = 0; fl < fn; ++fl) {
            const double2 t = tw[((f0 + fl) * k) & mask], q = sq[fl];
            gr = fma(-q.y, t.y, fma(q.x, t.x, gr));
            gi = fma(q.y, t.x, fma(q.x, t.y, gi));
        }
    }
    grid[(int64_t)g * nf + k] = make_double2(gr, gi);
}

// ---- type 2, step 3: workgroup (256 samples, column c) ---------------------------------------------------------------------------------
// grid[((c nb + j) ntw + twin) nf + k], ntw = 2 with the first-order twins
__global__ void __launch_bounds__(256)
eval_interp_kernel(const double *__restrict__ x, const double *__restrict__ v, const double *__restrict__ y, int64_t M, double a, double D_hi, double D_lo, int nf,
                   const double2 *__restrict__ grid, int twin, EvalBasis B, double scale, double *__restrict__ out, double *__restrict__ part, int64_t nslab) {
    __shared__ double red[256];
    const int64_t m = (int64_t)blockIdx.x * kEvalBlock + threadIdx.x;
    const bool valid = m < M;
    const int c = blockIdx.y, nb = B.nb, mask = nf - 1, ntw = twin ? 2 : 1;
    const double xv = valid ? x[m] : 0.0, vv = valid && B.vc ? v[m] : 0.0;
    int g0;
    const double p = nu_grid_pos(nu_phase_turns(D_hi, D_lo, xv), nf, &g0);
    double tap[kNuWidth];
#pragma unroll
    for (int k = 0; k < kNuWidth; ++k) tap[k] = nu_tap(g0, k, p);
    const int cell0 = (g0 + nf) & mask;
    double rc = 1.0, rs = 0.0;                                             // e^{i a x}
    if (a != 0.0) sincospi(2.0 * nu_phase_turns(a, 0.0, xv), &rs, &rc);
    const double ksum = B.vc && B.normalize ? eval_basis_sum(vv, B) : 1.0;
    double yh = 0.0;
    for (int j = 0; j < nb; ++j) {
        const double2 *g1 = grid + (int64_t)(c * nb + j) * ntw * nf;
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int k = 0; k < kNuWidth; ++k) {
            const double2 gv = g1[(cell0 + k) & mask];
            re = fma(tap[k], gv.x, re); im = fma(tap[k], gv.y, im);
        }
        if (twin) {                                                        // (uniform) + x * (the grid of i eps_f p_f)
            const double2 *g2 = g1 + nf;
            double re2 = 0.0, im2 = 0.0;
#pragma unroll
            for (int k = 0; k < kNuWidth; ++k) {
                const double2 gv = g2[(cell0 + k) & mask];
                re2 = fma(tap[k], gv.x, re2); im2 = fma(tap[k], gv.y, im2);
            }
            re = fma(xv, re2, re); im = fma(xv, im2, im);
        }
        yh = fma(eval_basis_value(vv, B, j, ksum), fma(-rs, im, rc * re), yh);
    }
    eval_store(yh, scale, y, m, valid, M, c, out, part, nslab, red);
}

// ---- the sums: workgroup = one of the 2 nc rows of slabs -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) eval_sums_kernel(const double *__restrict__ part, int64_t nslab, double *__restrict__ sums) {
    __shared__ double red[256];
    const double *p = part + (int64_t)blockIdx.x * nslab;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nslab; i += 256) s = s + p[i];
    const double r = eval_block_sum(s, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = r;
}

}  // namespace

int32_t launch_eval_direct(const double *x, const double *v, const double *y, int64_t M, const double *w_dev, int64_t Nf, const double *P_dev, int64_t nc,
                           const EvalBasis &B, double scale, double *out, double *part, hipStream_t s) {
    const EvalTiling t = eval_tiling(B.nb, nc);
    const dim3 grid((unsigned)eval_sum_slabs(M), (unsigned)t.cblocks);
    const int64_t nslab = eval_sum_slabs(M);
    const double2 *P = reinterpret_cast<const double2 *>(P_dev);
    if (t.tc == 1) hipLaunchKernelGGL(eval_direct_kernel<1>, grid, dim3(256), 0, s, x, v, y, M, w_dev, (int)Nf, P, (int)nc, B, scale, out, part, nslab);
    else if (t.tc == 4) hipLaunchKernelGGL(eval_direct_kernel<4>, grid, dim3(256), 0, s, x, v, y, M, w_dev, (int)Nf, P, (int)nc, B, scale, out, part, nslab);
    else hipLaunchKernelGGL(eval_direct_kernel<8>, grid, dim3(256), 0, s, x, v, y, M, w_dev, (int)Nf, P, (int)nc, B, scale, out, part, nslab);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

// grids_dev[ngrids][nf] (re, im) from Q_dev[ngrids][Nf]; tw_dev: nf (re, im) of scratch
int32_t launch_eval_grids(const double *Q_dev, int64_t ngrids, int64_t Nf, int nf, double *tw_dev, double *grids_dev, hipStream_t s) {
    double2 *tw = reinterpret_cast<double2 *>(tw_dev);
    hipLaunchKernelGGL(eval_twiddle_kernel, dim3((unsigned)(nf / 256)), dim3(256), 0, s, nf, tw);
    hipLaunchKernelGGL(eval_grid_kernel, dim3((unsigned)(nf / 256), (unsigned)ngrids), dim3(256), 0, s, reinterpret_cast<const double2 *>(Q_dev), (int)Nf, nf, tw,
                       reinterpret_cast<double2 *>(grids_dev));
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t launch_eval_interp(const double *x, const double *v, const double *y, int64_t M, double a, double D_hi, double D_lo, int nf, const double *grids_dev,
                           bool twin, int64_t nc, const EvalBasis &B, double scale, double *out, double *part, hipStream_t s) {
    hipLaunchKernelGGL(eval_interp_kernel, dim3((unsigned)eval_sum_slabs(M), (unsigned)nc), dim3(256), 0, s, x, v, y, M, a, D_hi, D_lo, nf,
                       reinterpret_cast<const double2 *>(grids_dev), twin ? 1 : 0, B, scale, out, part, eval_sum_slabs(M));
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

// sums_dev[2 c + {0, 1}] = sum, sum of squares of column c from part[2 nc][eval_sum_slabs(M)]
int32_t launch_eval_sums(const double *part, int64_t M, int64_t nc, double *sums_dev, hipStream_t s) {
    hipLaunchKernelGGL(eval_sums_kernel, dim3((unsigned)(2 * nc)), dim3(256), 0, s, part, eval_sum_slabs(M), sums_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace lpvs
