// lomb.hip -- the generalised Lomb-Scargle periodogram of non-uniformly sampled signals (lombscargle; hand-written HIP, gfx950).
//
// Per frequency f_k and signal c, with normalised weights w = W / sum W and phases phi = 2 pi f_k t_n:
//   C = sum w cos, S = sum w sin, C2 = sum w cos 2phi, S2 = sum w sin 2phi, YC = sum w y cos, YS = sum w y sin     (4 + 2 ns non-uniform Fourier sums)
// and the 2x2 / 3x3 least-squares fit of y ~ c + a cos + b sin in closed form (lomb_epilogue_kernel; include/lpvspectral.h has the formulas).
//
// PHASES.  The phase of (f, t) is that of the EXACT product f t: p = fl(f t), e = fma(f, t, -p) (error-free), and the turns
// (p - rint(p)) + e go to sincospi -- nothing grows with |f t|.
//
// DIRECT PATH (any grid): lomb_direct_kernel.  A workgroup = 64 frequencies x 4 sample lanes (lomb_plan.h: lomb_tiling) walks one slab of
// samples, staged through LDS 256 at a time; one sincospi per (sample, frequency), the double angle from c^2 - s^2 and 2 s c; 4 + 2 ts
// accumulators in registers.  The four lanes are added as (0 + 1) + (2 + 3), the slabs by a pairwise tree (lomb_slab_sum_kernel): a fixed
// order, so two calls give the same bits, and a signal's sums do not depend on which other signals ride along.
//
// TRANSFORM PATH (progressions, cut into blocks by lomb_plan.h): lomb_prephase_kernel forms a block's weight vectors
// w e^{i 2 pi base t}, w y_c e^{i 2 pi base t} (real and imaginary parts as separate real vectors), nufft.hip's spreading and mode
// extraction (launch_nufft_tab, as it is) transform them, and lomb_combine_kernel puts real and imaginary transforms back together,
// adds the first-order term of the frequency residuals from the t-weighted twins, and files the block's sums.
//
// MOMENTS: sum W, the weighted means and YY by slabs of 256 samples and a fixed tree (lomb_scan / lomb_mean / lomb_center kernels).
//
// WINDOWS (lombscargle_spectrogram / lombscargle_welch; include/lpvspectral.h g5): every window is the estimate above of its own samples
// with the weights W g, g a taper evaluated from time.  The lomb_windows_* kernels walk the work list of lomb_plan.h (one item per slab
// of a window; the slab is a constant, so a window's sums are added in an order that depends on that window alone): three moment passes,
// the segmented direct kernel (the inner loop of lomb_direct_kernel), a pairwise tree per window, the epilogue per (frequency, window,
// signal) and the average over the windows that are not empty.  lomb_time_windows_kernel: the index range of a time interval.
#include "lpvs_internal.h"
#include "lomb_plan.h"
#include "lomb_device.h"

namespace lpvs {
namespace {

// (lomb_block_sum, lomb_sincos, lomb_lane_sum, lomb_pairwise and lomb_fit: lomb_device.h, shared with lomb_boot.hip)
// ---- moments ---------------------------------------------------------------------------------------------------------------------------
// flags: bit 0 a non-finite t, y or W, bit 1 a negative weight (integer OR: order-free); part[workgroup] = sum of W over its 256 samples
__global__ void __launch_bounds__(256)
lomb_scan_kernel(const double *__restrict__ t, const double *__restrict__ y, const double *__restrict__ W, int64_t N, int ns, int *__restrict__ flags,
                 double *__restrict__ part) {
    __shared__ double red[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double wv = 0.0;
    int bad = 0;
    if (n < N) {
        const double inf = 1.0 / 0.0;
        wv = W ? W[n] : 1.0;
        if (!(fabs(t[n]) < inf) || !(fabs(wv) < inf)) bad |= 1;
        for (int c = 0; c < ns; ++c)
            if (!(fabs(y[(int64_t)c * N + n]) < inf)) bad |= 1;
        if (wv < 0.0) bad |= 2;
    }
    if (bad) atomicOr(flags, bad);
    const double s = lomb_block_sum(bad ? 0.0 : wv, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// out[row] = sum of part[row][0 .. nslab): thread t the slabs t, t + 256, ... ascending, then the tree
__global__ void __launch_bounds__(256) lomb_tree_kernel(const double *__restrict__ part, int64_t nslab, double *__restrict__ out) {
    __shared__ double red[256];
    const double *p = part + (int64_t)blockIdx.x * nslab;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nslab; i += 256) s = s + p[i];
    const double r = lomb_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}
// w = W / sum W (signal 0's workgroups write it); part[c][workgroup] = sum of w y_c
__global__ void __launch_bounds__(256)
lomb_mean_kernel(const double *__restrict__ y, const double *__restrict__ W, int64_t N, double sumW, double *__restrict__ w, double *__restrict__ part,
                 int64_t nslab) {
    __shared__ double red[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    double v = 0.0;
    if (n < N) {
        const double wv = (W ? W[n] : 1.0) / sumW;
        if (c == 0) w[n] = wv;
        v = wv * y[(int64_t)c * N + n];
    }
    const double s = lomb_block_sum(v, red);
    if (threadIdx.x == 0) part[(int64_t)c * nslab + blockIdx.x] = s;
}
// wy[c][n] = w (y_c - m_c), m_c = the weighted mean (center) or 0; part[2 c + {0, 1}][workgroup] = sum w yc, sum w yc^2 and
// part[2 ns + c][workgroup] = sum w y_c^2 of the signal as given (the scale of the constant-signal rule)
__global__ void __launch_bounds__(256)
lomb_center_kernel(const double *__restrict__ y, const double *__restrict__ w, int64_t N, const double *__restrict__ mean, int center,
                   double *__restrict__ wy, double *__restrict__ part, int64_t nslab) {
    __shared__ double red[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const double m = center ? mean[c] : 0.0;
    double v1 = 0.0, v2 = 0.0, v3 = 0.0;
    if (n < N) {
        const double yr = y[(int64_t)c * N + n], yc = yr - m;
        v1 = w[n] * yc;
        v2 = v1 * yc;
        v3 = (w[n] * yr) * yr;
        wy[(int64_t)c * N + n] = v1;
    }
    const double s1 = lomb_block_sum(v1, red), s2 = lomb_block_sum(v2, red), s3 = lomb_block_sum(v3, red);
    if (threadIdx.x == 0) {
        part[(int64_t)(2 * c) * nslab + blockIdx.x] = s1;
        part[(int64_t)(2 * c + 1) * nslab + blockIdx.x] = s2;
        part[(int64_t)(2 * gridDim.y + c) * nslab + blockIdx.x] = s3;
    }
}

// the inner loop of the direct kernels (lomb_direct_kernel and the segmented lomb_windows_direct_kernel): sample lane `lane` walks the
// staged samples lane, lane + 4, ... of one frequency: one sincospi per sample, the double angle from c^2 - s^2 and 2 s c
template <int TS>
__device__ inline void lomb_walk_stage(double fv, const double *st, const double *sw, const double (*swy)[LB_STAGE], int cnt, int lane, double *acc) {
    for (int i = lane; i < cnt; i += LB_LANES) {
        double sn, cs;
        lomb_sincos(fv, st[i], &sn, &cs);
        const double wv = sw[i];
        const double c2 = fma(cs, cs, -(sn * sn)), s2 = 2.0 * (sn * cs);
        acc[0] = fma(wv, cs, acc[0]);
        acc[1] = fma(wv, sn, acc[1]);
        acc[2] = fma(wv, c2, acc[2]);
        acc[3] = fma(wv, s2, acc[3]);
#pragma unroll
        for (int c = 0; c < TS; ++c) {
            const double v = swy[c][i];
            acc[4 + 2 * c] = fma(v, cs, acc[4 + 2 * c]);
            acc[5 + 2 * c] = fma(v, sn, acc[5 + 2 * c]);
        }
    }
}
// ---- direct path: workgroup (tile of 64 frequencies, slab of samples, block of TS signals) ---------------------------------------------
// part[(slab nrow + row) Nf + k], nrow = 4 + 2 ns: rows C, S, C2, S2 (written by signal block 0), then YC_c, YS_c
template <int TS>
__global__ void __launch_bounds__(256)
lomb_direct_kernel(const double *__restrict__ t, const double *__restrict__ w, const double *__restrict__ wy, int64_t N, int ns, const double *__restrict__ f,
                   int64_t Nf, int64_t slab_samples, double *__restrict__ part) {
    constexpr int NA = 4 + 2 * TS;
    __shared__ double st[LB_STAGE], sw[LB_STAGE], swy[TS][LB_STAGE];
    __shared__ double red[NA][LB_LANES][LB_TF];
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
        lomb_walk_stage<TS>(fv, st, sw, swy, cnt, lane, acc);
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) red[a][lane][fl] = acc[a];
    __syncthreads();
    if (lane != 0 || k >= Nf) return;
    const int nrow = 4 + 2 * ns;
    double *o = part + (int64_t)blockIdx.y * nrow * Nf + k;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const double v = lomb_lane_sum(red[a], fl);
        if (a < 4) { if (blockIdx.z == 0) o[(int64_t)a * Nf] = v; }
        else if (c0 + (a - 4) / 2 < ns) o[(int64_t)(4 + 2 * c0 + (a - 4)) * Nf] = v;
    }
}

// sums[e] = lomb_pairwise over the slabs of part[slab][e], e < nrow Nf
__global__ void __launch_bounds__(256) lomb_slab_sum_kernel(const double *__restrict__ part, int64_t nslab, int64_t count, double *__restrict__ sums) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    sums[e] = lomb_pairwise(part + e, count, nslab);
}

// ---- transform path ------------------------------------------------------------------------------------------------------------------------
// Wt[n][nq]: columns q < nre = 1 + g: {w, w y_c0, ...} cos(2 pi base t); with prephase, columns nre + q the same times sin
__global__ void __launch_bounds__(256)
lomb_prephase_kernel(const double *__restrict__ t, const double *__restrict__ w, const double *__restrict__ wy, int64_t N, int c0, int g, double base,
                     int prephase, double *__restrict__ Wt) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double sn = 0.0, cs = 1.0;
    if (prephase) lomb_sincos(base, t[n], &sn, &cs);
    const int nre = 1 + g, nq = prephase ? 2 * nre : nre;
    double *o = Wt + n * nq;
    for (int q = 0; q < nre; ++q) {
        const double v = q == 0 ? w[n] : wy[(int64_t)(c0 + q - 1) * N + n];
        o[q] = prephase ? v * cs : v;
        if (prephase) o[nre + q] = v * sn;
    }
}
// tab[(j nq + q) 4 + {cos, sin, t cos, t sin}] of a block -> sums[row][k0 + j]: Z = (A - B') + i (B + A') for the weight (re) + i (im) with
// transforms A + i B and A' + i B'; first-order term Z += i 2 pi e Zt, e = escale eps[k0 + j].  row0 < 0: column q goes to the rows of
// signal c0 + q - 1 (q = 0: rows 0, 1, C and S); row0 >= 0: the single column goes to rows row0, row0 + 1 (C2, S2).
__global__ void __launch_bounds__(256)
lomb_combine_kernel(const double *__restrict__ tab, int nq, int nre, int prephase, int count, int64_t k0, int64_t Nf, const double *__restrict__ eps, double escale,
                    int row0, int c0, double *__restrict__ sums) {
    const int j = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
    if (j >= count) return;
    const double *a = tab + ((int64_t)j * nq + q) * 4;
    double zr = a[0], zi = a[1], tr = a[2], ti = a[3];
    if (prephase) {
        const double *b = tab + ((int64_t)j * nq + nre + q) * 4;
        zr = zr - b[1]; zi = zi + b[0];
        tr = tr - b[3]; ti = ti + b[2];
    }
    const double e = escale * eps[k0 + j];
    if (e != 0.0) {
        const double h = 6.283185307179586 * e;
        zr = fma(-h, ti, zr);
        zi = fma(h, tr, zi);
    }
    const int row = row0 >= 0 ? row0 : (q == 0 ? 0 : 4 + 2 * (c0 + q - 1));
    sums[(int64_t)row * Nf + k0 + j] = zr;
    sums[(int64_t)(row + 1) * Nf + k0 + j] = zi;
}

// ---- epilogue: one thread per (frequency, signal) --------------------------------------------------------------------------------------
// mom[2 c + {0, 1}] = Y_c, YY_c of the (centred) signal, mom[2 ns + c] = sum w y_c^2 of the signal as given; mean[c]: its weighted mean.
__global__ void __launch_bounds__(256)
lomb_epilogue_kernel(const double *__restrict__ sums, int64_t Nf, int ns, const double *__restrict__ mom, const double *__restrict__ mean, int fit_mean,
                     int center, int psd, double Nsamples, double *__restrict__ power, double *__restrict__ coef, int *__restrict__ ndegenerate) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (k >= Nf) return;
    const LombFit r = lomb_fit(sums[k], sums[Nf + k], sums[2 * Nf + k], sums[3 * Nf + k], sums[(int64_t)(4 + 2 * c) * Nf + k], sums[(int64_t)(5 + 2 * c) * Nf + k],
                               mom[2 * c], mom[2 * c + 1], mom[2 * ns + c], center ? mean[c] : 0.0, fit_mean, center, psd, Nsamples);
    if (r.degenerate && c == 0) atomicAdd(ndegenerate, 1);
    power[(int64_t)c * Nf + k] = r.pw;
    if (coef) {
        const int64_t plane = Nf * ns;
        coef[(int64_t)c * Nf + k] = r.a;
        coef[plane + (int64_t)c * Nf + k] = r.b;
        coef[2 * plane + (int64_t)c * Nf + k] = r.c;
    }
}

// ---- windows: segmented kernels over the work list of lomb_plan.h (item = one slab of one window) -----------------------------------------
// The taper of the window [lo, hi] at time t: 1 (rect), or sin^2(pi u), u = (t - lo) / (hi - lo), 0 outside [0, 1] and 1 when hi == lo
// (hann).  The rounding of the quotient q = fl(d / L) is taken back to first order -- r = fma(-q, L, d) is its exact remainder, and
// sin pi (q + r / L) = sin pi q + pi cos pi q (r / L) -- so that what is left is the error of sincospi and of the square.
// It is evaluated where it is consumed, once per (window, sample) and pass; no array of sum(counts) tapers is kept.
__device__ inline double lomb_taper(int kind, double t, double lo, double hi) {
    if (kind == LPVS_TAPER_RECT) return 1.0;
    const double L = hi - lo;
    if (!(L > 0.0)) return 1.0;
    const double d = t - lo, q = d / L;
    if (!(q >= 0.0 && q <= 1.0)) return 0.0;
    const double r = fma(-q, L, d) / L;
    double sn, cs;
    sincospi(q, &sn, &cs);
    const double sv = fma(3.141592653589793 * cs, r, sn);
    return sv * sv;
}
// W g of sample n (an index into the record) of window w
__device__ inline double lomb_window_weight(const LombWindows &A, int w, int64_t n) {
    return (A.W ? A.W[n] : 1.0) * lomb_taper(A.taper, A.t[n], A.lo[w], A.hi[w]);
}
// the samples [n0, n1) of the record that item `item` covers
__device__ inline int lomb_item_range(const LombWindows &A, int64_t item, int64_t *n0, int64_t *n1) {
    const LombWindowItem it = A.items[item];
    const int64_t s0 = A.starts[it.window];
    *n0 = s0 + it.first; *n1 = s0 + it.last + 1;
    return it.window;
}
// The moments' kernels: one workgroup per item (and signal); it adds the item's blocks of 256 samples -- each by the tree over the
// threads -- in ascending order.  pass 0: part[item] = sum W g;  pass 1: part[item ns + c] = sum w y_c, w = W g / swg;
// pass 2: part[item 3 ns + {2 c, 2 c + 1, 2 ns + c}] = sum w yc, sum w yc^2, sum w y^2 (yc = y - the window's mean, or y)
template <int PASS>
__global__ void __launch_bounds__(256)
lomb_windows_moments_kernel(const LombWindows A, const double *__restrict__ swg, const double *__restrict__ mean, int center, double *__restrict__ part) {
    __shared__ double red[256];
    int64_t n0, n1;
    const int w = lomb_item_range(A, blockIdx.x, &n0, &n1);
    const int c = blockIdx.y;
    const double sw = PASS > 0 ? swg[w] : 1.0;
    const double m = PASS == 2 && center ? mean[(int64_t)w * A.ns + c] : 0.0;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int64_t base = n0; base < n1; base += 256) {
        const int64_t n = base + threadIdx.x;
        double v1 = 0.0, v2 = 0.0, v3 = 0.0;
        if (n < n1) {
            const double wg = lomb_window_weight(A, w, n);
            if (PASS == 0) v1 = wg;
            else {
                const double wv = sw > 0.0 ? wg / sw : 0.0, yr = A.y[(int64_t)c * A.N + n];
                if (PASS == 1) v1 = wv * yr;
                else {
                    const double yc = yr - m;
                    v1 = wv * yc;
                    v2 = v1 * yc;
                    v3 = (wv * yr) * yr;
                }
            }
        }
        const double s1 = lomb_block_sum(v1, red);
        a1 = base == n0 ? s1 : a1 + s1;
        if (PASS == 2) {
            const double s2 = lomb_block_sum(v2, red), s3 = lomb_block_sum(v3, red);
            a2 = base == n0 ? s2 : a2 + s2;
            a3 = base == n0 ? s3 : a3 + s3;
        }
    }
    if (threadIdx.x != 0) return;
    const int64_t item = blockIdx.x;
    if (PASS == 0) part[item] = a1;
    else if (PASS == 1) part[item * A.ns + c] = a1;
    else {
        double *o = part + item * 3 * A.ns;
        o[2 * c] = a1; o[2 * c + 1] = a2; o[2 * A.ns + c] = a3;
    }
}
// out[w rows + r] = the pairwise tree over the items of window w of part[item rows + r] (an empty window: 0); a thread per element
__global__ void __launch_bounds__(256)
lomb_windows_tree_kernel(const double *__restrict__ part, int64_t rows, const int64_t *__restrict__ offset, const int32_t *__restrict__ nslab, int64_t total,
                         double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t w = e / rows, r = e - w * rows;
    out[e] = lomb_pairwise(part + offset[w] * rows + r, rows, nslab[w]);
}
// The segmented direct kernel: workgroup = (item, tile of 64 frequencies) x block of TS signals, laid out as lomb_direct_kernel: 64 x 4
// threads, 256 samples staged through LDS at a time -- here with the weight W g / swg and the centred w (y - mean) formed while staging --
// the same accumulators and the same (0 + 1) + (2 + 3).  part[(item nrow + row) Nf + k]
template <int TS>
__global__ void __launch_bounds__(256)
lomb_windows_direct_kernel(const LombWindows A, const double *__restrict__ f, int64_t Nf, int64_t ftiles, const double *__restrict__ swg,
                           const double *__restrict__ mean, double *__restrict__ part) {
    constexpr int NA = 4 + 2 * TS;
    __shared__ double st[LB_STAGE], sw[LB_STAGE], swy[TS][LB_STAGE];
    __shared__ double red[NA][LB_LANES][LB_TF];
    const int fl = threadIdx.x % LB_TF, lane = threadIdx.x / LB_TF;
    const int64_t item = (int64_t)blockIdx.x / ftiles, tile = (int64_t)blockIdx.x - item * ftiles;
    const int64_t k = tile * LB_TF + fl;
    const int c0 = blockIdx.y * TS, ns = A.ns;
    const double fv = k < Nf ? f[k] : 0.0;
    int64_t n0, n1;
    const int w = lomb_item_range(A, item, &n0, &n1);
    const double sumwg = swg[w];
    double m[TS];
#pragma unroll
    for (int c = 0; c < TS; ++c) m[c] = mean && c0 + c < ns ? mean[(int64_t)w * ns + c0 + c] : 0.0;
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    for (int64_t base = n0; base < n1; base += LB_STAGE) {
        const int cnt = (int)(n1 - base < LB_STAGE ? n1 - base : LB_STAGE);
        __syncthreads();                                                   // the previous stage has been walked
        if ((int)threadIdx.x < cnt) {
            const int64_t n = base + threadIdx.x;
            const double wg = lomb_window_weight(A, w, n), wv = sumwg > 0.0 ? wg / sumwg : 0.0;
            st[threadIdx.x] = A.t[n];
            sw[threadIdx.x] = wv;
#pragma unroll
            for (int c = 0; c < TS; ++c) swy[c][threadIdx.x] = c0 + c < ns ? wv * (A.y[(int64_t)(c0 + c) * A.N + n] - m[c]) : 0.0;
        }
        __syncthreads();
        lomb_walk_stage<TS>(fv, st, sw, swy, cnt, lane, acc);
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) red[a][lane][fl] = acc[a];
    __syncthreads();
    if (lane != 0 || k >= Nf) return;
    const int nrow = 4 + 2 * ns;
    double *o = part + item * nrow * Nf + k;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const double v = lomb_lane_sum(red[a], fl);
        if (a < 4) { if (blockIdx.y == 0) o[(int64_t)a * Nf] = v; }
        else if (c0 + (a - 4) / 2 < ns) o[(int64_t)(4 + 2 * c0 + (a - 4)) * Nf] = v;
    }
}
// one thread per (frequency, window, signal): power[(c nwin + w) Nf + k], the planes of coef likewise.  An empty window (no samples, or
// weights that sum to 0) gives zeros and is reported in empty[w]; it counts no degenerate pairs.
__global__ void __launch_bounds__(256)
lomb_windows_epilogue_kernel(const LombWindows A, const double *__restrict__ sums, int64_t Nf, const double *__restrict__ swg, const double *__restrict__ mom,
                             const double *__restrict__ mean, int fit_mean, int center, int psd, double *__restrict__ power, double *__restrict__ coef,
                             int32_t *__restrict__ empty, int *__restrict__ flags, unsigned long long *__restrict__ ndegenerate) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, total = Nf * A.nwin * A.ns;
    if (e >= total) return;
    const int64_t k = e % Nf, w = (e / Nf) % A.nwin;
    const int c = (int)(e / (Nf * A.nwin)), ns = A.ns;
    const double sw = swg[w];
    const bool live = sw > 0.0;
    if (k == 0 && c == 0) {
        empty[w] = live ? 0 : 1;
        if (!(fabs(sw) < 1.0 / 0.0)) atomicOr(flags, 4);
    }
    LombFit r = {0.0, 0.0, 0.0, 0.0, false};
    if (live) {
        const double *s = sums + w * (4 + 2 * ns) * Nf + k, *mo = mom + w * 3 * ns;
        r = lomb_fit(s[0], s[Nf], s[2 * Nf], s[3 * Nf], s[(int64_t)(4 + 2 * c) * Nf], s[(int64_t)(5 + 2 * c) * Nf], mo[2 * c], mo[2 * c + 1], mo[2 * ns + c],
                     center ? mean[w * ns + c] : 0.0, fit_mean, center, psd, (double)A.counts[w]);
        if (r.degenerate && c == 0) atomicAdd(ndegenerate, 1ull);
    }
    power[e] = r.pw;
    if (coef) { coef[e] = r.a; coef[total + e] = r.b; coef[2 * total + e] = r.c; }
}
// out[c Nf + k] = the mean over the windows that are not empty of cols[(c nwin + w) Nf + k]: the pairwise tree of lomb_pairwise over
// those windows in the order of the list (a binary counter of partial sums), divided by their number; 0 if there is none
__global__ void __launch_bounds__(256)
lomb_windows_average_kernel(const double *__restrict__ cols, int64_t Nf, int64_t nwin, int64_t ns, const int32_t *__restrict__ empty, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Nf * ns) return;
    const int64_t k = e % Nf, c = e / Nf;
    double stack[26];                                                      // nwin <= kLombMaxWindows = 2^24
    int64_t j = 0;
    for (int64_t w = 0; w < nwin; ++w) {
        if (empty[w]) continue;
        double v = cols[(c * nwin + w) * Nf + k];
        int b = 0;
        for (; (j >> b) & 1; ++b) v = stack[b] + v;
        stack[b] = v;
        ++j;
    }
    double r = 0.0;
    bool have = false;
    for (int b = 0; b < 26; ++b)
        if ((j >> b) & 1) { r = have ? stack[b] + r : stack[b]; have = true; }
    out[e] = j > 0 ? r / (double)j : 0.0;
}
// time windows: is t finite and non-decreasing (flags), and one binary search per edge: edges[2 w] = #{t < lo_w}, edges[2 w + 1] = #{t <= hi_w}
__global__ void __launch_bounds__(256) lomb_sorted_kernel(const double *__restrict__ t, int64_t N, int *__restrict__ flags) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    int bad = 0;
    if (!(fabs(t[n]) < 1.0 / 0.0)) bad |= 1;
    if (n + 1 < N && t[n] > t[n + 1]) bad |= 8;
    if (bad) atomicOr(flags, bad);
}
__global__ void __launch_bounds__(256)
lomb_time_windows_kernel(const double *__restrict__ t, int64_t N, const double *__restrict__ lo, const double *__restrict__ hi, int64_t nwin, int64_t *__restrict__ edges) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * nwin) return;
    const bool upper = e & 1;
    const double v = upper ? hi[e >> 1] : lo[e >> 1];
    int64_t a = 0, b = N;                                                  // the answer lies in [a, b]
    while (a < b) {
        const int64_t mid = a + (b - a) / 2;
        const double tv = t[mid];
        if (upper ? tv <= v : tv < v) a = mid + 1; else b = mid;
    }
    edges[e] = a;
}

}  // namespace

// flags_dev: one int, zeroed here; sumW_dev: one double; part: lomb_sum_slabs(N) doubles
int32_t launch_lomb_scan(const double *t, const double *y, const double *W, int64_t N, int64_t ns, int *flags_dev, double *part, double *sumW_dev, hipStream_t s) {
    const int64_t nslab = lomb_sum_slabs(N);
    LPVS_HIP(hipMemsetAsync(flags_dev, 0, sizeof(int), s));
    hipLaunchKernelGGL(lomb_scan_kernel, dim3((unsigned)nslab), dim3(256), 0, s, t, y, W, N, (int)ns, flags_dev, part);
    hipLaunchKernelGGL(lomb_tree_kernel, dim3(1), dim3(256), 0, s, part, nslab, sumW_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// w[N], wy[ns][N], mean_dev[ns], mom_dev[3 ns] = {Y_c, YY_c} per signal, then sum w y_c^2 of the signals as given; part: 3 ns lomb_sum_slabs(N) doubles
int32_t launch_lomb_moments(const double *y, const double *W, int64_t N, int64_t ns, double sumW, bool center, double *w, double *wy, double *mean_dev,
                            double *mom_dev, double *part, hipStream_t s) {
    const int64_t nslab = lomb_sum_slabs(N);
    hipLaunchKernelGGL(lomb_mean_kernel, dim3((unsigned)nslab, (unsigned)ns), dim3(256), 0, s, y, W, N, sumW, w, part, nslab);
    hipLaunchKernelGGL(lomb_tree_kernel, dim3((unsigned)ns), dim3(256), 0, s, part, nslab, mean_dev);
    hipLaunchKernelGGL(lomb_center_kernel, dim3((unsigned)nslab, (unsigned)ns), dim3(256), 0, s, y, w, N, mean_dev, center ? 1 : 0, wy, part, nslab);
    hipLaunchKernelGGL(lomb_tree_kernel, dim3((unsigned)(3 * ns)), dim3(256), 0, s, part, nslab, mom_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// sums[(4 + 2 ns)][Nf] by direct summation; part: nslab (4 + 2 ns) Nf doubles
int32_t launch_lomb_direct(const double *t, const double *w, const double *wy, int64_t N, int64_t ns, const double *f_dev, int64_t Nf, const LombTiling &tl,
                           double *part, double *sums, hipStream_t s) {
    const dim3 grid((unsigned)tl.ftiles, (unsigned)tl.nslab, (unsigned)tl.sblocks);
    if (tl.ts == 1) hipLaunchKernelGGL(lomb_direct_kernel<1>, grid, dim3(256), 0, s, t, w, wy, N, (int)ns, f_dev, Nf, tl.slab_samples, part);
    else hipLaunchKernelGGL(lomb_direct_kernel<4>, grid, dim3(256), 0, s, t, w, wy, N, (int)ns, f_dev, Nf, tl.slab_samples, part);
    const int64_t count = (4 + 2 * ns) * Nf;
    hipLaunchKernelGGL(lomb_slab_sum_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, s, part, tl.nslab, count, sums);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// sums[e] = the pairwise tree over the slabs of part[slab][e], e < count (lomb_terms.hip adds its slabs with the same kernel)
int32_t launch_lomb_slab_sum(const double *part, int64_t nslab, int64_t count, double *sums, hipStream_t s) {
    hipLaunchKernelGGL(lomb_slab_sum_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, s, part, nslab, count, sums);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// Wt[N][nq], nq = lomb_weight_vectors(.., g, prephase): the weights of signals c0 .. c0 + g - 1 (g = 0: w alone) times e^{i 2 pi base t}
int32_t launch_lomb_prephase(const double *t, const double *w, const double *wy, int64_t N, int c0, int g, double base, bool prephase, double *Wt, hipStream_t s) {
    hipLaunchKernelGGL(lomb_prephase_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, t, w, wy, N, c0, g, base, prephase ? 1 : 0, Wt);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_lomb_combine(const double *tab, int nq, int nre, bool prephase, int count, int64_t k0, int64_t Nf, const double *eps_dev, double escale, int row0,
                            int c0, double *sums, hipStream_t s) {
    hipLaunchKernelGGL(lomb_combine_kernel, dim3((unsigned)ceil_div(count, 256), (unsigned)nre), dim3(256), 0, s, tab, nq, nre, prephase ? 1 : 0, count, k0, Nf,
                       eps_dev, escale, row0, c0, sums);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// power[ns][Nf] (column-major Nf x ns), coef[3][ns][Nf] or nullptr; ndeg_dev: one int, zeroed here
int32_t launch_lomb_epilogue(const double *sums, int64_t Nf, int64_t ns, const double *mom_dev, const double *mean_dev, bool fit_mean, bool center, bool psd,
                             int64_t N, double *power, double *coef, int *ndeg_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(ndeg_dev, 0, sizeof(int), s));
    hipLaunchKernelGGL(lomb_epilogue_kernel, dim3((unsigned)ceil_div(Nf, 256), (unsigned)ns), dim3(256), 0, s, sums, Nf, (int)ns, mom_dev, mean_dev,
                       fit_mean ? 1 : 0, center ? 1 : 0, psd ? 1 : 0, (double)N, power, coef, ndeg_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

// ---- windows -------------------------------------------------------------------------------------------------------------------------------
static void launch_lomb_windows_tree(const LombWindows &A, const double *part, int64_t rows, double *out, hipStream_t s) {
    const int64_t total = A.nwin * rows;
    hipLaunchKernelGGL(lomb_windows_tree_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, part, rows, A.offset, A.nslab, total, out);
}
int32_t launch_lomb_windows_moments(const LombWindows &A, bool center, double *swg, double *mean, double *mom, double *part, hipStream_t s) {
    const dim3 one((unsigned)A.nitems), per((unsigned)A.nitems, (unsigned)A.ns);
    const double *none = nullptr;
    if (A.nitems > 0) hipLaunchKernelGGL(lomb_windows_moments_kernel<0>, one, dim3(256), 0, s, A, none, none, 0, part);
    launch_lomb_windows_tree(A, part, 1, swg, s);
    if (A.nitems > 0) hipLaunchKernelGGL(lomb_windows_moments_kernel<1>, per, dim3(256), 0, s, A, (const double *)swg, none, 0, part);
    launch_lomb_windows_tree(A, part, A.ns, mean, s);
    if (A.nitems > 0) hipLaunchKernelGGL(lomb_windows_moments_kernel<2>, per, dim3(256), 0, s, A, (const double *)swg, (const double *)mean, center ? 1 : 0, part);
    launch_lomb_windows_tree(A, part, 3 * (int64_t)A.ns, mom, s);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_lomb_windows_direct(const LombWindows &A, const double *f_dev, int64_t Nf, const LombTiling &tl, const double *swg, const double *mean_or_null,
                                   double *part, double *sums, hipStream_t s) {
    const dim3 grid((unsigned)(A.nitems * tl.ftiles), (unsigned)tl.sblocks);
    if (A.nitems > 0) {
        if (tl.ts == 1) hipLaunchKernelGGL(lomb_windows_direct_kernel<1>, grid, dim3(256), 0, s, A, f_dev, Nf, tl.ftiles, swg, mean_or_null, part);
        else hipLaunchKernelGGL(lomb_windows_direct_kernel<4>, grid, dim3(256), 0, s, A, f_dev, Nf, tl.ftiles, swg, mean_or_null, part);
    }
    launch_lomb_windows_tree(A, part, (4 + 2 * (int64_t)A.ns) * Nf, sums, s);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_lomb_windows_epilogue(const LombWindows &A, const double *sums, int64_t Nf, const double *swg, const double *mom, const double *mean, bool fit_mean,
                                     bool center, bool psd, double *power, double *coef, int32_t *empty, int *flags_dev, unsigned long long *ndeg_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(ndeg_dev, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(lomb_windows_epilogue_kernel, dim3((unsigned)ceil_div(Nf * A.nwin * A.ns, 256)), dim3(256), 0, s, A, sums, Nf, swg, mom, mean,
                       fit_mean ? 1 : 0, center ? 1 : 0, psd ? 1 : 0, power, coef, empty, flags_dev, ndeg_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_lomb_windows_average(const double *cols, int64_t Nf, int64_t nwin, int64_t ns, const int32_t *empty, double *out, hipStream_t s) {
    hipLaunchKernelGGL(lomb_windows_average_kernel, dim3((unsigned)ceil_div(Nf * ns, 256)), dim3(256), 0, s, cols, Nf, nwin, ns, empty, out);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
int32_t launch_lomb_time_windows(const double *t, int64_t N, const double *lo, const double *hi, int64_t nwin, int *flags_dev, int64_t *edges, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(flags_dev, 0, sizeof(int), s));
    hipLaunchKernelGGL(lomb_sorted_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, t, N, flags_dev);
    hipLaunchKernelGGL(lomb_time_windows_kernel, dim3((unsigned)ceil_div(2 * nwin, 256)), dim3(256), 0, s, t, N, lo, hi, nwin, edges);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace lpvs
