// clean.hip -- CLEAN deconvolution of the spectra of unevenly sampled records (Roberts, Lehar & Dreher, AJ 93, 968, 1987): the kernels
// behind lpvs_dirty_spectrum_f64, lpvs_clean_loop_f64, lpvs_clean_restore_f64 and lpvs_clean_f64 (drivers: uneven.hip; the decisions:
// clean_plan.h; the definition: include/lpvspectral.h g11).
//
// The dirty spectrum and the spectral window are lomb.hip's sums C, S, YC, YS on the 2 Nf - 1 frequencies m df, repacked here:
// Wn_m = (C_m, -S_m), D_k = (YC_k, -YS_k).  The LOOP is one workgroup per signal and ONE launch for all iterations: an iteration is a
// dozen scalar flops every thread repeats for itself, one pass over the residual in which a thread updates its bins AND keeps the best
// admissible (P, k) of the new values, one arg-max over the workgroup and one barrier.  The peak's residual value travels with the
// arg-max, and bin k belongs to thread k mod threads throughout, so no thread reads a residual another one wrote -- the residual may
// live in LDS or in global memory behind the same pointer, with no fence.  The tie rule (the lowest index among equal P) makes the
// arg-max independent of the reduction's shape and of the thread count.  Every product and sum below is a rounded double operation in
// the order the header states (-ffp-contract=off; no explicit FMA in this file).  No floating-point atomics, no cooperative launch.
#include <climits>

#include "lpvs_internal.h"

namespace lpvs {

namespace {

constexpr int kNoBin = INT_MAX;

// is the candidate (P, k) ahead of the best so far (bP, bk)?  A NaN P is never ahead, and bP = -1 (nothing yet) loses to every P >= 0.
__device__ __forceinline__ bool clean_ahead(double P, int k, double bP, int bk) { return P > bP || (P == bP && k < bk); }

// ---- the dirty stage: rows of lomb.hip's sums -> interleaved complex spectra --------------------------------------------------------------
// sums[(4 + 2 ns)][M], M = 2 Nf - 1: rows C, S, C2, S2, then YC_c, YS_c.  Wn[M], D[ns][Nf].
__global__ void __launch_bounds__(256)
clean_repack_kernel(const double *__restrict__ sums, int64_t M, int64_t Nf, int ns, double *__restrict__ Wn, double *__restrict__ D) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    Wn[2 * m] = sums[m];
    Wn[2 * m + 1] = -sums[M + m];
    if (m >= Nf) return;
    for (int c = 0; c < ns; ++c) {
        D[2 * ((int64_t)c * Nf + m)] = sums[(4 + 2 * (int64_t)c) * M + m];
        D[2 * ((int64_t)c * Nf + m) + 1] = -sums[(5 + 2 * (int64_t)c) * M + m];
    }
}

// flags |= 1 where x holds a value that is not finite (the family's flag word)
__global__ void __launch_bounds__(256) clean_finite_kernel(const double *__restrict__ x, int64_t count, int *__restrict__ flags) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) bad = bad || !isfinite(x[i]);
    if (bad) atomicOr(flags, 1);
}

// ---- the prologue: den_p = 1 - (Re Wn_2p^2 + Im Wn_2p^2), mask_p = den_p >= 2^-20, and the count of the admissible bins ------------------------
__global__ void __launch_bounds__(256)
clean_prologue_kernel(const double *__restrict__ Wn, int64_t Nf, double *__restrict__ den, unsigned char *__restrict__ mask, int *__restrict__ nadm) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= Nf) return;
    const double wr = Wn[4 * p], wi = Wn[4 * p + 1];
    const double d = 1.0 - (wr * wr + wi * wi);
    const bool ok = d >= kCleanMinDen;
    den[p] = d;
    mask[p] = ok ? 1 : 0;
    if (ok) atomicAdd(nadm, 1);
}

// ---- the loop -----------------------------------------------------------------------------------------------------------------------------
struct CleanLoopArgs {
    const double *D, *Wn, *den;
    const unsigned char *mask;
    int Nf, niter, use_lds;
    double gain, tol;
    double *R, *C, *pickval;
    int32_t *picks, *iters, *status;
};

// The workgroup's best admissible (P, k) with the residual (re, im) at k: every thread brings its own best and leaves with the
// workgroup's.  A butterfly over the wave, one slot per wave in the set `par` of the two, ONE barrier, and every thread folds the slots.
__device__ __forceinline__ void clean_argmax(double (*slots)[16][4], int par, int nwaves, double &bP, int &bk, double &bre, double &bim) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double myre = bre, myim = bim;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oP = __shfl_xor(bP, off, 64);
        const int ok = __shfl_xor(bk, off, 64);
        if (clean_ahead(oP, ok, bP, bk)) { bP = oP; bk = ok; }
    }
    // the wave's best is the own best of the lane that holds bin bk: bk mod threads mod 64 = bk mod 64 (threads is a multiple of 64)
    const int owner = bk == kNoBin ? 0 : (bk & 63);
    const double wre = __shfl(myre, owner, 64), wim = __shfl(myim, owner, 64);
    if (lane == 0) {
        slots[par][wave][0] = bP; slots[par][wave][1] = wre; slots[par][wave][2] = wim; slots[par][wave][3] = bk == kNoBin ? -1.0 : (double)bk;
    }
    __syncthreads();
    bP = -1.0; bk = kNoBin; bre = 0.0; bim = 0.0;
    for (int w = 0; w < nwaves; ++w) {
        const double sP = slots[par][w][0], sk = slots[par][w][3];
        if (sk < 0.0) continue;
        if (clean_ahead(sP, (int)sk, bP, bk)) { bP = sP; bk = (int)sk; bre = slots[par][w][1]; bim = slots[par][w][2]; }
    }
}

__global__ void __launch_bounds__(kCleanMaxThreads) clean_loop_kernel(CleanLoopArgs A) {
    extern __shared__ double clean_residual[];                       // [Nf][2] when A.use_lds
    __shared__ double slots[2][16][4];                               // kCleanSlotBytes
    const int c = blockIdx.x, tid = threadIdx.x, T = blockDim.x, nwaves = T >> 6, Nf = A.Nf;
    const double *__restrict__ Dc = A.D + 2 * (size_t)c * Nf;
    const double *__restrict__ Wn = A.Wn;
    double *Rg = A.R + 2 * (size_t)c * Nf, *Cc = A.C + 2 * (size_t)c * Nf;
    double *R = A.use_lds ? clean_residual : Rg;
    // R = D, and the first search
    double bP = -1.0, bre = 0.0, bim = 0.0;
    int bk = kNoBin;
    for (int k = tid; k < Nf; k += T) {
        const double re = Dc[2 * k], im = Dc[2 * k + 1];
        R[2 * k] = re; R[2 * k + 1] = im;
        if (A.mask[k]) {
            const double P = re * re + im * im;
            if (clean_ahead(P, k, bP, bk)) { bP = P; bk = k; bre = re; bim = im; }
        }
    }
    int it = 0, status = kCleanStatusNiter;
    double thr = 0.0;
    for (; it < A.niter; ++it) {
        clean_argmax(slots, it & 1, nwaves, bP, bk, bre, bim);
        if (bk == kNoBin) { status = kCleanStatusEmpty; break; }
        if (it == 0) thr = (A.tol * A.tol) * bP;
        if (A.tol > 0.0 && bP <= thr) { status = kCleanStatusTol; break; }
        // the component at the peak p: a = (R_p - conj(R_p) Wn_2p) / den_p, c = gain a  (every thread, the same bits)
        const int p = bk;
        const double w2r = Wn[4 * (size_t)p], w2i = Wn[4 * (size_t)p + 1], dn = A.den[p];
        const double tr = bre * w2r + bim * w2i, ti = bre * w2i - bim * w2r;
        const double ar = (bre - tr) / dn, ai = (bim - ti) / dn;
        const double cr = A.gain * ar, ci = A.gain * ai;
        if (tid == 0) {
            Cc[2 * p] = Cc[2 * p] + cr; Cc[2 * p + 1] = Cc[2 * p + 1] + ci;
            const size_t q = (size_t)c * A.niter + it;
            A.picks[q] = p; A.pickval[2 * q] = cr; A.pickval[2 * q + 1] = ci;
        }
        // R_k -= c Wn_{k-p} + conj(c) Wn_{k+p}, Wn_{-m} = conj(Wn_m); and the search of the next iteration in the same pass
        bP = -1.0; bk = kNoBin; bre = 0.0; bim = 0.0;
        for (int k = tid; k < Nf; k += T) {
            const int m1 = k - p, a1 = m1 < 0 ? -m1 : m1, m2 = k + p;
            const double w1r = Wn[2 * (size_t)a1], w1s = Wn[2 * (size_t)a1 + 1], w1i = m1 < 0 ? -w1s : w1s;
            const double x2r = Wn[2 * (size_t)m2], x2i = Wn[2 * (size_t)m2 + 1];
            const double ur = (cr * w1r - ci * w1i) + (cr * x2r + ci * x2i);
            const double ui = (cr * w1i + ci * w1r) + (cr * x2i - ci * x2r);
            const double re = R[2 * k] - ur, im = R[2 * k + 1] - ui;
            R[2 * k] = re; R[2 * k + 1] = im;
            if (A.mask[k]) {
                const double P = re * re + im * im;
                if (clean_ahead(P, k, bP, bk)) { bP = P; bk = k; bre = re; bim = im; }
            }
        }
    }
    if (A.use_lds)
        for (int k = tid; k < Nf; k += T) { Rg[2 * k] = R[2 * k]; Rg[2 * k + 1] = R[2 * k + 1]; }     // (a thread's own bins)
    if (tid == 0) { A.iters[c] = it; A.status[c] = status; }
}

// ---- restoration ---------------------------------------------------------------------------------------------------------------------------
// list[c][0 .. count_c - 1]: the bins p with C_p != 0 of signal c, in increasing p (an ordered compaction: ballots and counts, no atomics)
__global__ void __launch_bounds__(256) clean_compact_kernel(const double *__restrict__ C, int Nf, int32_t *__restrict__ list, int32_t *__restrict__ count) {
    __shared__ int wsum[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *Cc = C + 2 * (size_t)c * Nf;
    int32_t *lc = list + (size_t)c * Nf;
    int base = 0;
    for (int k0 = 0; k0 < Nf; k0 += 256) {
        const int k = k0 + tid;
        const bool flag = k < Nf && (Cc[2 * k] != 0.0 || Cc[2 * k + 1] != 0.0);
        const unsigned long long b = __ballot(flag);
        const int rank = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        if (flag) lc[base + before + rank] = k;
        base += total;
        __syncthreads();
    }
    if (tid == 0) count[c] = base;
}

// the beam: B_m = exp(-(x x) / two_s2), x = (double)m df, two_s2 = 2 (sigma sigma); m = 0 .. 2 Nf - 2
__global__ void __launch_bounds__(256) clean_beam_kernel(int64_t M, double df, double two_s2, double *__restrict__ B) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const double x = (double)m * df;
    B[m] = exp(-(x * x) / two_s2);
}

// S_k = R_k + sum over the list, in increasing p, of C_p B_{k-p} + conj(C_p) B_{k+p}: one thread per k, a gather
__global__ void __launch_bounds__(256)
clean_restore_kernel(const double *__restrict__ R, const double *__restrict__ C, int Nf, const int32_t *__restrict__ list, const int32_t *__restrict__ count,
                     const double *__restrict__ B, double *__restrict__ S) {
    const int c = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Nf) return;
    const double *Cc = C + 2 * (size_t)c * Nf;
    const int32_t *lc = list + (size_t)c * Nf;
    const int n = count[c];
    double sr = R[2 * ((size_t)c * Nf + k)], si = R[2 * ((size_t)c * Nf + k) + 1];
    for (int j = 0; j < n; ++j) {
        const int p = lc[j], d = k < p ? p - k : k - p;
        const double cr = Cc[2 * p], ci = Cc[2 * p + 1], b1 = B[d], b2 = B[k + p];
        sr = sr + (cr * b1 + cr * b2);
        si = si + (ci * b1 - ci * b2);
    }
    S[2 * ((size_t)c * Nf + k)] = sr;
    S[2 * ((size_t)c * Nf + k) + 1] = si;
}

}  // namespace

int32_t launch_clean_repack(const double *sums, int64_t Nf, int64_t ns, double *Wn, double *D, hipStream_t s) {
    const int64_t M = 2 * Nf - 1;
    clean_repack_kernel<<<dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, s>>>(sums, M, Nf, (int)ns, Wn, D);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t launch_clean_finite(const double *x, int64_t count, int *flags_dev, hipStream_t s) {
    if (count <= 0) return LPVS_OK;
    const int64_t blocks = ceil_div(count, 256);
    clean_finite_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s>>>(x, count, flags_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t launch_clean_prologue(const double *Wn, int64_t Nf, double *den, unsigned char *mask, int *nadm_dev, hipStream_t s) {
    LPVS_HIP(hipMemsetAsync(nadm_dev, 0, sizeof(int), s));
    clean_prologue_kernel<<<dim3((unsigned)ceil_div(Nf, 256)), dim3(256), 0, s>>>(Wn, Nf, den, mask, nadm_dev);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t launch_clean_loop(const double *D, const double *Wn, const double *den, const unsigned char *mask, int64_t ns, int64_t Nf, double gain, int64_t niter,
                          double tol, const CleanPlan &plan, double *R, double *C, int32_t *picks, double *pickval, int32_t *iters, int32_t *status, hipStream_t s) {
    CleanLoopArgs A;
    A.D = D; A.Wn = Wn; A.den = den; A.mask = mask;
    A.Nf = (int)Nf; A.niter = (int)niter; A.use_lds = plan.residual == kCleanResidualLds;
    A.gain = gain; A.tol = tol;
    A.R = R; A.C = C; A.pickval = pickval; A.picks = picks; A.iters = iters; A.status = status;
    const size_t lds = A.use_lds ? sizeof(double) * 2 * (size_t)Nf : 0;
    LPVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&clean_loop_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCleanLdsBudget));
    clean_loop_kernel<<<dim3((unsigned)ns), dim3((unsigned)plan.threads), lds, s>>>(A);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t launch_clean_restore(const double *R, const double *C, int64_t ns, int64_t Nf, double df, double sigma, int32_t *list, int32_t *count, double *beam,
                             double *S, hipStream_t s) {
    const int64_t M = 2 * Nf - 1;
    clean_compact_kernel<<<dim3((unsigned)ns), dim3(256), 0, s>>>(C, (int)Nf, list, count);
    LPVS_HIP(hipGetLastError());
    clean_beam_kernel<<<dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, s>>>(M, df, 2.0 * (sigma * sigma), beam);
    LPVS_HIP(hipGetLastError());
    clean_restore_kernel<<<dim3((unsigned)ceil_div(Nf, 256), (unsigned)ns), dim3(256), 0, s>>>(R, C, (int)Nf, list, count, beam, S);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

}  // namespace lpvs
