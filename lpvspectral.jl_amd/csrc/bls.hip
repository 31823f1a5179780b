// bls.hip -- the box least squares periodogram of non-uniformly sampled signals (bls; Kovacs, Zucker & Mazeh, A&A 391, 369, 2002, in its
// binned form; hand-written HIP, gfx950; the definition: include/lpvspectral.h g9; the decisions and the error model: bls_plan.h;
// DESIGN.md 4.17).
//
// QUANTISE: bls_max_kernel leaves A_c = max_n |wy_c[n]| per signal -- a block maximum, then an integer atomicMax on the bit pattern of the
// non-negative double (order-preserving, exact and order-free) -- and the largest term of YY_c the same way; the host turns them into
// the shifts (bls_plan.h: bls_shift_y), and bls_quantise_kernel writes qy_c[n] = rint(wy_c[n] 2^shy_c) and qw[n] = rint(w[n] 2^60) as
// 64-bit integers and adds YY_c = sum wy (y - ybar) up as two integer words per term (bls_plan.h: bls_yy_words): order-free as well.  (A maximum over the grid
// has to be complete before the first sample is quantised: two launches, since no workgroup waits for another.)
//
// FOLD AND SEARCH: bls_kernel<F, TS, UNIT>, one launch per pass of TS signals, one workgroup of 256 threads per F frequencies.
//   zero     the histograms of the workgroup in LDS: per frequency TS rows of 64-bit sums of qy, one of qw (not with UNIT) and 32-bit counts
//   stage    the samples in blocks of 256, one per thread, held in registers: t, qw, qy of the pass's signals
//   fold     per (sample, frequency): p = f t, e = fma(f, t, -p), phi = (p - rint(p)) + e, + 1 if negative; bin = min(nbins - 1,
//            (int)floor(phi nbins)); 64-bit integer LDS atomic adds (32-bit for the count): exact, so the order of the samples is immaterial
//   prefix   every histogram becomes its inclusive prefix sum in place (a wave per row: 64 contiguous chunks, a shuffle scan of the chunk
//            totals); the raw histograms are written out first when the caller asked for them
//   search   a thread owns the start bins tid, tid + 256, ... and loops over the widths; a box is two LDS reads per row; the objective of
//            bls_plan.h from the exact integers; the best box per signal under the tie rule (largest, then narrowest, then earliest)
//   arg-max  over the workgroup with the same rule: shuffles within a wave, four candidates through LDS
//   write    thread 0 forms depth, depth_err and the power of the best box and writes the (frequency, signal) entry of every plane
// No cooperative launch, no spin-wait, nothing crosses workgroups but the degenerate counter (an integer atomic add).
#include "lpvs_internal.h"
#include "bls_plan.h"
#include "fold_device.h"

namespace lpvs {
namespace {

typedef unsigned long long u64;

// amax[c] = the bit pattern of max_n |wy[c][n]| and amax[ns + c] that of max_n v_n, v_n = wy[c][n] (y[c][n] - m_c) >= 0, the terms of YY_c
// (zeroed by the launcher; the bits of non-negative doubles order as the doubles do)
__global__ void __launch_bounds__(256)
bls_max_kernel(const double *__restrict__ y, const double *__restrict__ wy, const double *__restrict__ mean, int center, int64_t N, int ns, u64 *__restrict__ amax) {
    __shared__ double red[256], redv[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const double m = center ? mean[c] : 0.0;
    const double a = n < N ? wy[(int64_t)c * N + n] : 0.0;
    red[threadIdx.x] = fabs(a);
    redv[threadIdx.x] = n < N ? a * (y[(int64_t)c * N + n] - m) : 0.0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
            redv[threadIdx.x] = fmax(redv[threadIdx.x], redv[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(&amax[c], (u64)__double_as_longlong(red[0]));
        atomicMax(&amax[ns + c], (u64)__double_as_longlong(fabs(redv[0])));
    }
}

// rows 0 .. ns - 1: qy[c][n] = rint(wy[c][n] 2^shy[c]) (0 where amax[c] = 0: the constant signal), and the two integer words of YY_c
// (bls_plan.h: bls_yy_words) added up -- within the workgroup in LDS, then one integer atomic add per word: exact, whatever the order;
// row ns (weights only): qw[n] = rint(w[n] 2^60).  shy[ns + c]: the shift of the terms of YY_c (kBlsNoShift: nothing is added)
__global__ void __launch_bounds__(256)
bls_quantise_kernel(const double *__restrict__ y, const double *__restrict__ w, const double *__restrict__ wy, const double *__restrict__ mean, int center, int64_t N,
                    int ns, int log2n, const int32_t *__restrict__ shy, const u64 *__restrict__ amax, long long *__restrict__ qw, long long *__restrict__ qy,
                    long long *__restrict__ yyacc) {
    __shared__ long long rhi[256], rlo[256];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (c >= ns) {
        if (n < N) qw[n] = bls_quantise(w[n], kBlsWeightShift);
        return;
    }
    long long hi = 0, lo = 0;
    const int shv = shy[ns + c];
    if (n < N) {
        const double a = wy[(int64_t)c * N + n];
        qy[(int64_t)c * N + n] = amax[c] == 0 ? 0 : bls_quantise(a, shy[c]);
        if (shv != kBlsNoShift) bls_yy_words(a * (y[(int64_t)c * N + n] - (center ? mean[c] : 0.0)), shv, log2n, &hi, &lo);
    }
    rhi[threadIdx.x] = hi; rlo[threadIdx.x] = lo;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { rhi[threadIdx.x] += rhi[threadIdx.x + s]; rlo[threadIdx.x] += rlo[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0 && shv != kBlsNoShift) {
        atomicAdd(reinterpret_cast<u64 *>(&yyacc[2 * c]), (u64)rhi[0]);
        atomicAdd(reinterpret_cast<u64 *>(&yyacc[2 * c + 1]), (u64)rlo[0]);
    }
}

// candidate (d, k, b) against the best so far (bd, bk, bb); a width of 0 is "none"
__device__ inline bool bls_better(double d, int k, int b, double bd, int bk, int bb) {
    if (k == 0) return false;
    if (bk == 0) return true;
    return d > bd || (d == bd && (k < bk || (k == bk && b < bb)));
}

template <int F, int TS, bool UNIT>
__global__ void __launch_bounds__(256) bls_kernel(const BlsArgs A, int c0) {
    constexpr int NR = TS + (UNIT ? 0 : 1);                                // 64-bit rows per frequency: qy of the TS signals, then qw
    extern __shared__ u64 lds[];
    __shared__ double red_d[4];
    __shared__ int red_k[4], red_b[4];
    const int nb = A.nbins, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ns = A.ns;
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
    // ---- search
    for (int j = 0; j < F && k0 + j < A.Nf; ++j) {
        const int64_t kf = k0 + j;
        const long long *IY = reinterpret_cast<const long long *>(H) + j * NR * nb, *IW = IY + TS * nb;
        const unsigned int *IC = HC + j * nb;
        const int kmin = A.kmin[kf], kmax = A.kmax[kf];
        const long long Rq = UNIT ? (long long)N : IW[nb - 1];
        const unsigned int Ctot = IC[nb - 1];
        long long Sq[TS];
        double cS[TS], bd[TS];
        int bk[TS], bb[TS];
#pragma unroll
        for (int c = 0; c < TS; ++c) {
            Sq[c] = IY[c * nb + nb - 1];
            const double Sd = (double)Sq[c];
            cS[c] = (Sd * Sd) / (double)Rq;
            bd[c] = 0.0; bk[c] = 0; bb[c] = 0;
        }
        for (int b = tid; b < nb; b += 256) {
            const unsigned int cbefore = b > 0 ? IC[b - 1] : 0u;
            const long long wbefore = UNIT || b == 0 ? 0 : IW[b - 1];
            long long ybefore[TS];
#pragma unroll
            for (int c = 0; c < TS; ++c) ybefore[c] = b > 0 ? IY[c * nb + b - 1] : 0;
            for (int k = kmin; k <= kmax; ++k) {
                const long long cnt = (long long)bls_box<unsigned int>(IC, nb, b, k, cbefore, Ctot);
                if (cnt < A.min_count || N - cnt < A.min_count) continue;
                const long long rq = UNIT ? cnt : bls_box<long long>(IW, nb, b, k, wbefore, Rq), rcq = Rq - rq;
                if (rq <= 0 || rcq <= 0) continue;
                const double rd = (double)rq, rcd = (double)rcq;
#pragma unroll
                for (int c = 0; c < TS; ++c) {
                    const long long sq = bls_box<long long>(IY + c * nb, nb, b, k, ybefore[c], Sq[c]), scq = Sq[c] - sq;
                    if (A.dips_only && !((__int128)sq * rcq < (__int128)scq * rq)) continue;
                    const double sd = (double)sq, scd = (double)scq;
                    const double d = ((sd * sd) / rd + (scd * scd) / rcd) - cS[c];
                    if (bls_better(d, k, b, bd[c], bk[c], bb[c])) { bd[c] = d; bk[c] = k; bb[c] = b; }
                }
            }
        }
        // ---- arg-max per signal, then the entry of every plane
#pragma unroll
        for (int c = 0; c < TS; ++c) {
            if (c0 + c >= ns) continue;                                    // (uniform over the workgroup)
            double d = bd[c];
            int k = bk[c], b = bb[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double od = __shfl_down(d, off, 64);
                const int ok = __shfl_down(k, off, 64), ob = __shfl_down(b, off, 64);
                if (lane + off < 64 && bls_better(od, ok, ob, d, k, b)) { d = od; k = ok; b = ob; }
            }
            __syncthreads();                                               // (red_* of the previous signal have been read)
            if (lane == 0) { red_d[wave] = d; red_k[wave] = k; red_b[wave] = b; }
            __syncthreads();
            if (tid != 0) continue;
            for (int v = 1; v < 4; ++v)
                if (bls_better(red_d[v], red_k[v], red_b[v], d, k, b)) { d = red_d[v]; k = red_k[v]; b = red_b[v]; }
            const int cg = c0 + c;
            const int64_t o = (int64_t)cg * A.Nf + kf;
            const int shv = A.shy[ns + cg];
            const double Rg = A.mom[2 * ns + cg];
            const double YY = shv != kBlsNoShift ? bls_yy(A.yyacc[2 * cg], A.yyacc[2 * cg + 1], shv, A.log2n) : A.amax[ns + cg] == 0 ? 0.0 : 1.0 / 0.0;
            const double noise = lomb_yy_noise((double)N, A.center != 0, false, Rg, YY);
            const int shy = A.shy[cg];
            const double inf = 1.0 / 0.0;
            double delta = 0.0;
            if (k > 0) {
                const double dpos = d > 0.0 ? d : 0.0;
                delta = UNIT ? scalbn(dpos * (double)N, -2 * shy) : scalbn(dpos, kBlsWeightShift - 2 * shy);
            }
            const bool live = k > 0 && A.amax[cg] != 0 && YY > noise && YY < inf && delta < inf;
            double pw = 0.0, depth = 0.0, derr = 0.0;
            long long cnt = 0;
            if (live) {
                const unsigned int cbefore = b > 0 ? IC[b - 1] : 0u;
                cnt = (long long)bls_box<unsigned int>(IC, nb, b, k, cbefore, Ctot);
                const long long rq = UNIT ? cnt : bls_box<long long>(IW, nb, b, k, b > 0 ? IW[b - 1] : 0, Rq), rcq = Rq - rq;
                const long long sq = bls_box<long long>(IY + c * nb, nb, b, k, b > 0 ? IY[c * nb + b - 1] : 0, Sq[c]), scq = Sq[c] - sq;
                const double rd = UNIT ? (double)rq / (double)N : scalbn((double)rq, -kBlsWeightShift);
                const double rcd = UNIT ? (double)rcq / (double)N : scalbn((double)rcq, -kBlsWeightShift);
                depth = scalbn((double)scq / rcd - (double)sq / rd, -shy);
                derr = sqrt((1.0 / rd + 1.0 / rcd) / A.sumW);
                pw = A.chi2 ? A.sumW * delta : fmin(1.0, delta / YY);
            } else {
                atomicAdd(A.ndeg, 1ull);
            }
            A.power[o] = pw;
            A.depth[o] = depth;
            A.depth_err[o] = derr;
            A.start[o] = live ? b : 0;
            A.width[o] = live ? k : 0;
            A.count[o] = cnt;
            A.degenerate[o] = live ? 0 : 1;
        }
        __syncthreads();                                                   // (thread 0 has read red_* and the prefix sums of this frequency)
    }
}

template <int F, int TS>
int32_t bls_launch_unit(const BlsArgs &A, bool unit, int c0, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(A.Nf, F));
    if (unit) hipLaunchKernelGGL((bls_kernel<F, TS, true>), grid, dim3(256), lds, s, A, c0);
    else hipLaunchKernelGGL((bls_kernel<F, TS, false>), grid, dim3(256), lds, s, A, c0);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
template <int F>
int32_t bls_launch_ts(const BlsArgs &A, int ts, bool unit, int c0, size_t lds, hipStream_t s) {
    switch (ts) {
    case 1: return bls_launch_unit<F, 1>(A, unit, c0, lds, s);
    case 2: return bls_launch_unit<F, 2>(A, unit, c0, lds, s);
    case 4: return bls_launch_unit<F, 4>(A, unit, c0, lds, s);
    default: set_error("bls: no kernel for %d signals per pass", ts); return LPVS_EUNSUPPORTED;
    }
}

}  // namespace

// amax_dev[2 ns] = the bit patterns of max_n |wy[c][n]|, then of the largest term of YY_c: zeroed here
int32_t launch_bls_max(const double *y, const double *wy, const double *mean_dev, bool center, int64_t N, int64_t ns, unsigned long long *amax_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(amax_dev, 0, sizeof(unsigned long long) * (size_t)(2 * ns), s));
    hipLaunchKernelGGL(bls_max_kernel, dim3((unsigned)ceil_div(N, 256), (unsigned)ns), dim3(256), 0, s, y, wy, mean_dev, center ? 1 : 0, N, (int)ns, amax_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// qy[ns][N], with weights (qw != nullptr) qw[N], and yyacc_dev[2 ns] = the two integer words of every YY_c (zeroed here); shy_dev[2 ns]
int32_t launch_bls_quantise(const double *y, const double *w, const double *wy, const double *mean_dev, bool center, int64_t N, int64_t ns, int log2n,
                            const int32_t *shy_dev, const unsigned long long *amax_dev, long long *qw, long long *qy, long long *yyacc_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(yyacc_dev, 0, sizeof(long long) * (size_t)(2 * ns), s));
    hipLaunchKernelGGL(bls_quantise_kernel, dim3((unsigned)ceil_div(N, 256), (unsigned)(ns + (qw ? 1 : 0))), dim3(256), 0, s, y, w, wy, mean_dev, center ? 1 : 0, N,
                       (int)ns, log2n, shy_dev, amax_dev, qw, qy, yyacc_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}
// one launch per pass of plan.ts signals; A.ndeg: zeroed here
int32_t launch_bls(const BlsArgs &A, const BlsPlan &plan, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(A.ndeg, 0, sizeof(unsigned long long), s));
    const size_t lds = (size_t)plan.lds_bytes;
    for (int pass = 0; pass < plan.passes; ++pass) {
        const int c0 = pass * plan.ts;
        switch (plan.F) {
        case 1: LPVS_TRY(bls_launch_ts<1>(A, plan.ts, plan.unit != 0, c0, lds, s)); break;
        case 2: LPVS_TRY(bls_launch_ts<2>(A, plan.ts, plan.unit != 0, c0, lds, s)); break;
        case 4: LPVS_TRY(bls_launch_ts<4>(A, plan.ts, plan.unit != 0, c0, lds, s)); break;
        default: set_error("bls: no kernel for %d frequencies per workgroup", plan.F); return LPVS_EUNSUPPORTED;
        }
    }
    return LPVS_OK;
}

}  // namespace lpvs
