// cnormal.hip -- ComplexNormal sampling and the Monte-Carlo bands of the SpectralExt recipe on gfx950
// (src/utilities.jl:80-174, src/plotting.jl:54-97).
//
//   1. Cholesky       V = U'U of a symmetric positive definite f64 matrix, upper factor, blocked right-looking with panels of 128:
//                     the diagonal block is factored by one workgroup in LDS, the block row right of it is solved by forward
//                     substitution (one thread per column, its solution in LDS), the trailing upper triangle takes the rank-128 update
//                     on v_mfma_f64_16x16x4_f64 in 64 x 64 tiles.  Only the upper triangle of V is read (Hermitian(...) is :U).
//                     Every element is a fixed-order chain of fused multiply-adds: bit-reproducible, no atomics.
//   2. normals        Philox4x32-10, key = the 64-bit seed, counter = (row, column pair); Box-Muller in f64 on 2 x 53 bits.
//                     Element (i, j) depends on (seed, i, j) only.
//   3. sampling       Z = m' .+ R U, 256 columns x 64 draws per workgroup on the f64 MFMA, the k loop stops at the tile's last column
//                     (U is upper triangular); R is generated into LDS chunk by chunk when the caller supplies none.
//   4. bands          one workgroup per (frequency j, grid point i): d = dot(z[iMC, j:Nf:end], phi_i) for every draw, |d| (then
//                     angle(d)) as sortable keys in LDS, a bitonic sort, two order statistics and the fixed-order mean.
//   5. covariance     cov of a tall matrix with few columns (the sample-matrix constructors): two fixed-order block reductions.
#include "lpvs_internal.h"
#include "philox.h"

#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

namespace lpvs {
namespace {

constexpr int kNB = 128;            // panel width of the factorisation
constexpr int kLdT = kNB + 1;       // LDS leading dimension of the diagonal block
constexpr int kDiagBlock = 512;     // threads of the diagonal block's workgroup: 4 per column
constexpr int kSR = 64, kSC = 256, kKC = 16, kPadS = 16;   // sampling tile: draws x columns, k chunk, LDS row padding
constexpr int kBandBlock = 512;
constexpr int64_t kMaxDraws = 16384;   // keys of one cell in LDS: 16384 * 8 B = 128 KiB of the 160 KiB
constexpr int64_t kMaxBasis = 1024;    // phi of one grid point next to them
constexpr int kCovBlocks = 256, kCovMaxCols = 64;

typedef double d4 __attribute__((ext_vector_type(4)));

int32_t need_device() {
    if (lpvs_device_count() == 0) { set_error("no HIP device visible (the gfx950 path has no CPU fallback)"); return LPVS_EDEVICE; }
    return LPVS_OK;
}

// ---- 1. Cholesky ----------------------------------------------------------------------------------------------------------------------
// W (np x np, column-major, np % 128 == 0): upper triangle of V, identity on the padding, zero elsewhere
__global__ void __launch_bounds__(256) pad_upper_kernel(const double *V, int64_t n2, double *W, int64_t np) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= np * np) return;
    const int64_t r = idx % np, c = idx / np;
    W[idx] = (r <= c && c < n2) ? V[c * n2 + r] : (r == c ? 1.0 : 0.0);
}

// status[0]: 0, or 1 + the index of the first pivot that is not positive; every later kernel of the factorisation returns at once then.
// Step j: row j is scaled, then thread (column c, quarter q) takes rows j+1+q, j+5+q, ... <= c of column c of the trailing block.
__global__ void __launch_bounds__(kDiagBlock) chol_diag_kernel(double *W, int64_t np, int64_t k0, int *status) {
    extern __shared__ double T[];   // T[c * kLdT + r], upper triangle
    if (status[0]) return;
    const int tid = threadIdx.x, c = tid & (kNB - 1), q = tid / kNB;
    for (int idx = tid; idx < kNB * kNB; idx += kDiagBlock) {
        const int r = idx % kNB, cc = idx / kNB;
        T[cc * kLdT + r] = r <= cc ? W[(k0 + cc) * np + k0 + r] : 0.0;
    }
    __syncthreads();
    bool failed = false;
    for (int j = 0; j < kNB; ++j) {
        const double d = T[j * kLdT + j];
        if (!(d > 0.0)) { failed = true; if (tid == 0) status[0] = (int)(k0 + j) + 1; break; }   // the same value in every thread
        const double rj = sqrt(d);
        __syncthreads();
        if (q == 0 && c >= j) T[c * kLdT + j] = c == j ? rj : T[c * kLdT + j] / rj;
        __syncthreads();
        if (c > j) {   // A22[i][c] -= U[j][i] U[j][c], j < i <= c
            const double ujc = T[c * kLdT + j];
            for (int i = j + 1 + q; i <= c; i += kDiagBlock / kNB) T[c * kLdT + i] = fma(-T[i * kLdT + j], ujc, T[c * kLdT + i]);
        }
        __syncthreads();
    }
    if (failed) return;
    for (int idx = tid; idx < kNB * kNB; idx += kDiagBlock) {
        const int r = idx % kNB, cc = idx / kNB;
        W[(k0 + cc) * np + k0 + r] = r <= cc ? T[cc * kLdT + r] : 0.0;
    }
}

// U12 = U11^-T A12: column x of the block row solves U11' x = a by forward substitution, one thread per column, its solution in LDS
__global__ void __launch_bounds__(64) chol_panel_kernel(double *W, int64_t np, int64_t k0, const int *status) {
    extern __shared__ double X[];   // X[k * 64 + thread]
    if (status[0]) return;
    const int tid = threadIdx.x;
    const int64_t c = k0 + kNB + (int64_t)blockIdx.x * 64 + tid;
    if (c >= np) return;
    double *col = W + c * np + k0;
    for (int i = 0; i < kNB; ++i) {
        const double *u = W + (k0 + i) * np + k0;   // column i of U11 (the same address in every thread)
        double acc = col[i];
        for (int k = 0; k < i; ++k) acc = fma(-u[k], X[k * 64 + tid], acc);
        const double x = acc / u[i];
        X[i * 64 + tid] = x;
        col[i] = x;
    }
}

// A22 -= U12' U12 on the upper triangle, 64 x 64 tiles, one 32 x 32 quarter per wave.  The product is formed transposed
// (A operand: the tile's columns, B operand: its rows) so that the 16 lanes of a result register are adjacent in memory.
__global__ void __launch_bounds__(256) chol_trail_kernel(double *W, int64_t np, int64_t k0, const int *status) {
    if (status[0]) return;
    const int64_t ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    const int64_t base = k0 + kNB;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const int64_t i0 = base + ti * 64 + (wave >> 1) * 32, j0 = base + tj * 64 + (wave & 1) * 32;
    const double *P = W + k0;   // U12[k][col] = P[col * np + k]
    d4 acc[2][2];
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    for (int kk = 0; kk < kNB / 4; ++kk) {
        const int k = 4 * kk + lk;
        double opj[2], opi[2];
        for (int a = 0; a < 2; ++a) { opj[a] = P[(j0 + 16 * a + li) * np + k]; opi[a] = P[(i0 + 16 * a + li) * np + k]; }
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(opj[a], opi[b], acc[a][b], 0, 0, 0);
    }
    // C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15 (row i of the tile), row = (lane >> 4) + 4 reg (column j of the tile)
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int r = 0; r < 4; ++r) {
                double *dst = W + (j0 + 16 * a + lk + 4 * r) * np + (i0 + 16 * b + li);
                *dst = *dst - acc[a][b][r];
            }
}

__global__ void __launch_bounds__(256) extract_upper_kernel(const double *W, int64_t np, int64_t n2, double *U) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n2 * n2) return;
    const int64_t r = idx % n2, c = idx / n2;
    U[idx] = r <= c ? W[c * np + r] : 0.0;
}
__global__ void __launch_bounds__(256) zero_lower_kernel(double *W, int64_t np) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= np * np) return;
    if (idx % np > idx / np) W[idx] = 0.0;
}

// V (device, n2 x n2) -> W (np x np, upper factor above the diagonal; the strict lower triangle holds scratch)
int32_t factor_device(const double *V, int64_t n2, DevBuf &W, int64_t *np_out, hipStream_t s) {
    const int64_t np = round_up(n2, kNB);
    *np_out = np;
    DevBuf st;
    LPVS_TRY(W.alloc(sizeof(double) * (size_t)np * (size_t)np));
    LPVS_TRY(st.alloc(sizeof(int)));
    DrainOnExit drain(s);
    LPVS_HIP(hipMemsetAsync(st.p, 0, sizeof(int), s));
    const unsigned all = (unsigned)ceil_div(np * np, 256);
    pad_upper_kernel<<<all, 256, 0, s>>>(V, n2, W.as<double>(), np);
    LPVS_HIP(hipGetLastError());
    const size_t lds_diag = sizeof(double) * kNB * kLdT, lds_panel = sizeof(double) * kNB * 64;
    LPVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&chol_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_diag));
    LPVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&chol_panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_panel));
    for (int64_t k0 = 0; k0 < np; k0 += kNB) {
        chol_diag_kernel<<<1, kDiagBlock, lds_diag, s>>>(W.as<double>(), np, k0, st.as<int>());
        LPVS_HIP(hipGetLastError());
        const int64_t rest = np - k0 - kNB;
        if (rest <= 0) break;
        chol_panel_kernel<<<(unsigned)(rest / 64), 64, lds_panel, s>>>(W.as<double>(), np, k0, st.as<int>());
        LPVS_HIP(hipGetLastError());
        const unsigned T = (unsigned)(rest / 64);
        chol_trail_kernel<<<dim3(T, T), 256, 0, s>>>(W.as<double>(), np, k0, st.as<int>());
        LPVS_HIP(hipGetLastError());
    }
    int bad = 0;
    LPVS_TRY(copy_from_device(&bad, st.p, sizeof(int), s));
    if (bad) {
        set_error("matrix is not positive definite: pivot %d (0-based) is not positive (PosDefException)", bad - 1);
        return LPVS_ENUMERIC;
    }
    return LPVS_OK;
}

// ---- 2. normals -------------------------------------------------------------------------------------------------------------------------
// (philox4x32_10: philox.h, shared with the resampling indices of lomb_boot.hip)
// the two normals of (row, column pair): columns 2 pair and 2 pair + 1
__device__ inline void normal_pair(uint64_t seed, uint64_t row, uint64_t pair, double *z0, double *z1) {
    const U4 u = philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), (uint32_t)pair, (uint32_t)(pair >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t a = ((uint64_t)(u.w[0] >> 5) << 26) | (u.w[1] >> 6), b = ((uint64_t)(u.w[2] >> 5) << 26) | (u.w[3] >> 6);
    const double u1 = (double)(a + 1) * 0x1p-53;   // (0, 1]
    const double v2 = (double)b * 0x1p-52;         // 2 u2 in [0, 2), exact
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(v2, &sn, &cs);
    *z0 = r * cs;
    *z1 = r * sn;
}

__global__ void __launch_bounds__(256) randn_kernel(uint64_t seed, int64_t row0, int64_t rows, int64_t cols, double *R) {
    const int64_t pairs = (cols + 1) / 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * pairs) return;
    const int64_t i = idx % rows, p = idx / rows;
    double z0, z1;
    normal_pair(seed, (uint64_t)(row0 + i), (uint64_t)p, &z0, &z1);
    R[(2 * p) * rows + i] = z0;
    if (2 * p + 1 < cols) R[(2 * p + 1) * rows + i] = z1;
}

// ---- 3. sampling --------------------------------------------------------------------------------------------------------------------------
// Z[d][c] = m[c] + sum_{k <= c} R[d][k] U[k][c].  Transposed product (A operand: U', B operand: R') so that the lanes of a result
// register are adjacent draws of one column of Z (column-major).
__global__ void __launch_bounds__(256) cn_sample_kernel(const double *U, int64_t np, int64_t n2, const double *mvec, const double *R,
                                                        int64_t ldr, uint64_t seed, int64_t s, double *Z, int64_t ldz) {
    __shared__ double Rs[kKC][kSR + kPadS];
    __shared__ double Us[kKC][kSC + kPadS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * kSR, c0 = (int64_t)blockIdx.y * kSC;
    const int64_t kend = c0 + kSC < np ? c0 + kSC : np;
    d4 acc[4][4];
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < kend; k0 += kKC) {
        if (R) {
            for (int q = 0; q < kSR * kKC / 256; ++q) {
                const int idx = tid + 256 * q, row = idx & (kSR - 1), kk = idx / kSR;
                const int64_t gr = r0 + row, gk = k0 + kk;
                Rs[kk][row] = (gr < s && gk < n2) ? R[gk * ldr + gr] : 0.0;
            }
        } else {
            for (int q = 0; q < kSR * kKC / 2 / 256; ++q) {
                const int idx = tid + 256 * q, row = idx & (kSR - 1), pp = idx / kSR;
                const int64_t gk = k0 + 2 * pp;
                double z0, z1;
                normal_pair(seed, (uint64_t)(r0 + row), (uint64_t)(gk >> 1), &z0, &z1);
                Rs[2 * pp][row] = gk < n2 ? z0 : 0.0;
                Rs[2 * pp + 1][row] = gk + 1 < n2 ? z1 : 0.0;
            }
        }
        {
            const int64_t c = c0 + tid;
            for (int kk = 0; kk < kKC; ++kk) Us[kk][tid] = c < np ? U[c * np + k0 + kk] : 0.0;
        }
        __syncthreads();
        for (int k4 = 0; k4 < kKC / 4; ++k4) {
            const int k = 4 * k4 + lk;
            double opu[4], opr[4];
            for (int a = 0; a < 4; ++a) { opu[a] = Us[k][wave * 64 + 16 * a + li]; opr[a] = Rs[k][16 * a + li]; }
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(opu[a], opr[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
    for (int a = 0; a < 4; ++a)
        for (int r = 0; r < 4; ++r) {
            const int64_t c = c0 + wave * 64 + 16 * a + lk + 4 * r;
            if (c >= n2) continue;
            const double mc = mvec[c];
            for (int b = 0; b < 4; ++b) {
                const int64_t d = r0 + 16 * b + li;
                if (d < s) Z[c * ldz + d] = mc + acc[a][b][r];
            }
        }
}

// ---- 4. bands -----------------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long sort_key(double v) {   // IEEE bits that order as unsigned integers (negative values: all bits flipped)
    unsigned long long k;
    memcpy(&k, &v, 8);
    return (k >> 63) ? ~k : (k | 0x8000000000000000ull);
}
__device__ inline double sort_val(unsigned long long k) {
    k = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    memcpy(&v, &k, 8);
    return v;
}

// out: 6 planes of Nf x G (column-major): lower, upper, mean of |d|, then of angle(d)
__global__ void __launch_bounds__(kBandBlock) cn_bands_kernel(const double *Z, int64_t ldz, int64_t n, int64_t Nf, int64_t nb, const double *Phi,
                                                              int64_t G, int64_t nMC, int64_t P2, int32_t phase, int64_t il, int64_t iu,
                                                              double *out) {
    extern __shared__ unsigned long long keys[];   // P2 keys, then nb doubles of phi, then kBandBlock doubles of the reduction
    double *phi = reinterpret_cast<double *>(keys + P2), *red = phi + nb;
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x % G, j = blockIdx.x / G;   // grid points of one frequency are neighbours: they read the same columns of Z
    for (int64_t v = tid; v < nb; v += kBandBlock) phi[v] = Phi[v * G + i];
    __syncthreads();
    for (int pass = 0; pass <= (phase ? 1 : 0); ++pass) {
        double sum = 0.0;
        for (int64_t d = tid; d < P2; d += kBandBlock) {
            unsigned long long key = ~0ull;
            if (d < nMC) {
                double re = 0.0, im = 0.0;   // dot(z, phi) conjugates z (src/plotting.jl:81,83)
                for (int64_t v = 0; v < nb; ++v) {
                    const int64_t c = j + v * Nf;
                    re = fma(Z[c * ldz + d], phi[v], re);
                    im = fma(-Z[(n + c) * ldz + d], phi[v], im);
                }
                const double val = pass == 0 ? hypot(re, im) : atan2(im, re);
                sum += val;
                key = sort_key(val);
            }
            keys[d] = key;
        }
        __syncthreads();
        for (int64_t k = 2; k <= P2; k <<= 1)
            for (int64_t jj = k >> 1; jj > 0; jj >>= 1) {
                for (int64_t t = tid; t < P2 / 2; t += kBandBlock) {
                    const int64_t a = (t / jj) * 2 * jj + t % jj, b = a + jj;
                    const unsigned long long ka = keys[a], kb = keys[b];
                    if ((ka > kb) == ((a & k) == 0)) { keys[a] = kb; keys[b] = ka; }
                }
                __syncthreads();
            }
        red[tid] = sum;
        __syncthreads();
        for (int w = kBandBlock / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] = red[tid] + red[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            double *o = out + (size_t)(3 * pass) * Nf * G + i * Nf + j;
            o[0] = sort_val(keys[il]);
            o[(size_t)Nf * G] = sort_val(keys[iu]);
            o[2 * (size_t)Nf * G] = red[0] / (double)nMC;
        }
        __syncthreads();
    }
}

// ---- 5. covariance of a tall matrix -------------------------------------------------------------------------------------------------------
__device__ inline double block_sum256(double v, double *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}
// part[col * kCovBlocks + block] = sum of the block's rows of column col
__global__ void __launch_bounds__(256) cov_sums_kernel(const double *A, int64_t rows, double *part) {
    __shared__ double red[256];
    const int64_t col = blockIdx.y, chunk = (rows + kCovBlocks - 1) / kCovBlocks, lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < rows ? lo + chunk : rows;
    double acc = 0.0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += 256) acc += A[col * rows + r];
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) part[col * kCovBlocks + blockIdx.x] = acc;
}
// pair p = (a <= b) in column-major order of the upper triangle: part[p * kCovBlocks + block] = sum (A[r,a] - mean_a)(A[r,b] - mean_b)
__global__ void __launch_bounds__(256) cov_pairs_kernel(const double *A, int64_t rows, const double *mean, double *part) {
    __shared__ double red[256];
    int64_t b = 0, p = blockIdx.y;
    while (p > b) { p -= b + 1; ++b; }
    const int64_t a = p;
    const double ma = mean[a], mb = mean[b];
    const int64_t chunk = (rows + kCovBlocks - 1) / kCovBlocks, lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < rows ? lo + chunk : rows;
    double acc = 0.0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += 256) acc = fma(A[a * rows + r] - ma, A[b * rows + r] - mb, acc);
    acc = block_sum256(acc, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * kCovBlocks + blockIdx.x] = acc;
}

// ---- the handle ---------------------------------------------------------------------------------------------------------------------------
struct Cn {
    int device = 0;
    int64_t n = 0, n2 = 0, np = 0;
    DevBuf U, m;   // U: np x np, strict lower triangle zero, identity on the padding; m: [re; im]
};
std::mutex g_mu;
std::map<int64_t, std::unique_ptr<Cn>> g_handles;
int64_t g_next = 1;

Cn *find_cn(int64_t id) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_handles.find(id);
    if (it == g_handles.end()) { set_error("unknown ComplexNormal handle %lld", (long long)id); return nullptr; }
    return it->second.get();
}

// [0] factor, [1] sample, [2] bands, [3] total (ms); [4] 2n, [5] draws, [6] cells
thread_local double g_timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// Z (device, s x n2, ld s) = m' .+ R U
int32_t sample_device(const Cn &cn, int64_t s, uint64_t seed, const double *R, double *Z, hipStream_t st) {
    Staged<double> dR;
    if (R) LPVS_TRY(dR.set(R, s * cn.n2, cn.device, st));
    DrainOnExit drain(st);
    const dim3 grid((unsigned)ceil_div(s, kSR), (unsigned)ceil_div(cn.n2, kSC));
    cn_sample_kernel<<<grid, 256, 0, st>>>(cn.U.as<double>(), cn.np, cn.n2, cn.m.as<double>(), R ? dR.p : nullptr, s, seed, s, Z, s);
    LPVS_HIP(hipGetLastError());
    return LPVS_OK;
}

int32_t out_copy(double *dst, const double *src_dev, size_t count, hipStream_t s) {
    if (is_device_ptr(dst)) {
        LPVS_HIP(hipMemcpyAsync(dst, src_dev, sizeof(double) * count, hipMemcpyDefault, s));
        LPVS_HIP(hipStreamSynchronize(s));
        return LPVS_OK;
    }
    return copy_from_device(dst, src_dev, sizeof(double) * count, s);
}

int32_t cholesky_impl(const double *V, int64_t n2, int32_t device, double *U_out) {
    if (!V || !U_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (n2 < 1) { set_error("n2 must be positive, got %lld", (long long)n2); return LPVS_EARGUMENT; }
    LPVS_TRY(need_device());
    LPVS_HIP(hipSetDevice(device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    Staged<double> dV;
    DevBuf W, Uc;
    DrainOnExit drain(sh.s);
    LPVS_TRY(dV.set(V, n2 * n2, device, sh.s));
    int64_t np = 0;
    LPVS_TRY(factor_device(dV.p, n2, W, &np, sh.s));
    LPVS_TRY(Uc.alloc(sizeof(double) * (size_t)n2 * (size_t)n2));
    extract_upper_kernel<<<(unsigned)ceil_div(n2 * n2, 256), 256, 0, sh.s>>>(W.as<double>(), np, n2, Uc.as<double>());
    LPVS_HIP(hipGetLastError());
    return out_copy(U_out, Uc.as<double>(), (size_t)n2 * (size_t)n2, sh.s);
}

int32_t randn_impl(int64_t seed, int64_t row0, int64_t rows, int64_t cols, int32_t device, double *R_out) {
    if (!R_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (row0 < 0 || rows < 1 || cols < 1) { set_error("randn: row0 >= 0, rows >= 1, cols >= 1 are needed"); return LPVS_EARGUMENT; }
    LPVS_TRY(need_device());
    LPVS_HIP(hipSetDevice(device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    DevBuf Rd;
    DrainOnExit drain(sh.s);
    const bool direct = device_of_ptr(R_out) == device;
    if (!direct) LPVS_TRY(Rd.alloc(sizeof(double) * (size_t)rows * (size_t)cols));
    double *dst = direct ? R_out : Rd.as<double>();
    randn_kernel<<<(unsigned)ceil_div(rows * ((cols + 1) / 2), 256), 256, 0, sh.s>>>((uint64_t)seed, row0, rows, cols, dst);
    LPVS_HIP(hipGetLastError());
    if (!direct) return out_copy(R_out, dst, (size_t)rows * (size_t)cols, sh.s);
    LPVS_HIP(hipStreamSynchronize(sh.s));
    return LPVS_OK;
}

int32_t cov_impl(const double *A, int64_t rows, int64_t cols, int32_t device, double *mean_out, double *C_out) {
    if (!A || !mean_out || !C_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (rows < 2 || cols < 1 || cols > kCovMaxCols) { set_error("cov: at least 2 rows and 1 .. %d columns are needed, got %lld x %lld", kCovMaxCols, (long long)rows, (long long)cols); return LPVS_EARGUMENT; }
    if (is_device_ptr(mean_out) || is_device_ptr(C_out)) { set_error("cov: mean_out and C_out are host arrays"); return LPVS_EARGUMENT; }
    LPVS_TRY(need_device());
    LPVS_HIP(hipSetDevice(device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    Staged<double> dA;
    DevBuf part, dmean;
    DrainOnExit drain(sh.s);
    LPVS_TRY(dA.set(A, rows * cols, device, sh.s));
    const int64_t pairs = cols * (cols + 1) / 2;
    LPVS_TRY(part.alloc(sizeof(double) * (size_t)pairs * kCovBlocks));
    LPVS_TRY(dmean.alloc(sizeof(double) * (size_t)cols));
    std::vector<double> h((size_t)pairs * kCovBlocks);
    cov_sums_kernel<<<dim3(kCovBlocks, (unsigned)cols), 256, 0, sh.s>>>(dA.p, rows, part.as<double>());
    LPVS_HIP(hipGetLastError());
    LPVS_TRY(copy_from_device(h.data(), part.p, sizeof(double) * (size_t)cols * kCovBlocks, sh.s));
    for (int64_t c = 0; c < cols; ++c) {
        double acc = 0.0;
        for (int b = 0; b < kCovBlocks; ++b) acc += h[(size_t)c * kCovBlocks + b];
        mean_out[c] = acc / (double)rows;
    }
    LPVS_TRY(copy_to_device(dmean.p, mean_out, sizeof(double) * (size_t)cols, sh.s));
    cov_pairs_kernel<<<dim3(kCovBlocks, (unsigned)pairs), 256, 0, sh.s>>>(dA.p, rows, dmean.as<double>(), part.as<double>());
    LPVS_HIP(hipGetLastError());
    LPVS_TRY(copy_from_device(h.data(), part.p, sizeof(double) * h.size(), sh.s));
    int64_t p = 0;
    for (int64_t b = 0; b < cols; ++b)
        for (int64_t a = 0; a <= b; ++a, ++p) {
            double acc = 0.0;
            for (int k = 0; k < kCovBlocks; ++k) acc += h[(size_t)p * kCovBlocks + k];
            C_out[a + b * cols] = C_out[b + a * cols] = acc / (double)(rows - 1);   // corrected, as Statistics.cov
        }
    return LPVS_OK;
}

int32_t cn_create_impl(const double *m_re, const double *m_im, const double *V, int64_t n, int32_t device, int64_t *id) {
    if (!m_re || !m_im || !V || !id) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (n < 1) { set_error("n must be positive, got %lld", (long long)n); return LPVS_EARGUMENT; }
    LPVS_TRY(need_device());
    LPVS_HIP(hipSetDevice(device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    Events<4> ev;
    for (auto &x : ev.e) LPVS_HIP(hipEventCreate(&x));
    std::unique_ptr<Cn> cn(new Cn);
    cn->device = device; cn->n = n; cn->n2 = 2 * n;
    Staged<double> dV;
    DrainOnExit drain(sh.s);
    LPVS_TRY(dV.set(V, cn->n2 * cn->n2, device, sh.s));
    LPVS_HIP(hipEventRecord(ev.e[0], sh.s));
    LPVS_TRY(factor_device(dV.p, cn->n2, cn->U, &cn->np, sh.s));
    zero_lower_kernel<<<(unsigned)ceil_div(cn->np * cn->np, 256), 256, 0, sh.s>>>(cn->U.as<double>(), cn->np);
    LPVS_HIP(hipGetLastError());
    LPVS_HIP(hipEventRecord(ev.e[1], sh.s));
    LPVS_TRY(cn->m.alloc(sizeof(double) * (size_t)cn->n2));
    LPVS_TRY(copy_to_device(cn->m.p, m_re, sizeof(double) * (size_t)n, sh.s));
    LPVS_TRY(copy_to_device(cn->m.as<double>() + n, m_im, sizeof(double) * (size_t)n, sh.s));
    LPVS_HIP(hipStreamSynchronize(sh.s));
    float ms = 0;
    LPVS_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    for (double &t : g_timing) t = 0;
    g_timing[0] = ms; g_timing[3] = ms; g_timing[4] = (double)cn->n2;
    std::lock_guard<std::mutex> lk(g_mu);
    *id = g_next++;
    g_handles[*id] = std::move(cn);
    return LPVS_OK;
}

int32_t cn_rand_impl(int64_t id, int64_t s, int64_t seed, const double *R, double *Z_re, double *Z_im) {
    if (!Z_re || !Z_im) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (s < 1) { set_error("the number of draws must be positive, got %lld", (long long)s); return LPVS_EARGUMENT; }
    Cn *cn = find_cn(id);
    if (!cn) return LPVS_EARGUMENT;
    LPVS_HIP(hipSetDevice(cn->device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    Events<4> ev;
    for (auto &x : ev.e) LPVS_HIP(hipEventCreate(&x));
    DevBuf Z;
    DrainOnExit drain(sh.s);
    LPVS_TRY(Z.alloc(sizeof(double) * (size_t)s * (size_t)cn->n2));
    LPVS_HIP(hipEventRecord(ev.e[0], sh.s));
    LPVS_TRY(sample_device(*cn, s, (uint64_t)seed, R, Z.as<double>(), sh.s));
    LPVS_HIP(hipEventRecord(ev.e[1], sh.s));
    // complex(z[:, 1:n], z[:, n+1:end]) (src/utilities.jl:173): the two halves of the column-major s x 2n result
    LPVS_TRY(out_copy(Z_re, Z.as<double>(), (size_t)s * (size_t)cn->n, sh.s));
    LPVS_TRY(out_copy(Z_im, Z.as<double>() + (size_t)s * (size_t)cn->n, (size_t)s * (size_t)cn->n, sh.s));
    float ms = 0;
    LPVS_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    g_timing[1] = ms; g_timing[2] = 0; g_timing[3] = ms; g_timing[4] = (double)cn->n2; g_timing[5] = (double)s; g_timing[6] = 0;
    return LPVS_OK;
}

int32_t cn_bands_impl(int64_t id, int64_t Nf, int64_t nb, const double *Phi_g, int64_t G, int64_t nMC, int64_t seed, const double *R,
                      int32_t phase, double *Fl, double *Fu, double *Fm, double *Pl, double *Pu, double *Pm) {
    if (!Phi_g || !Fl || !Fu || !Fm || (phase && (!Pl || !Pu || !Pm))) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (Nf < 1 || nb < 1 || G < 1) { set_error("Nf, nb and G must be positive"); return LPVS_EARGUMENT; }
    if (nMC < 10) { set_error("nMC must be at least 10 (the lower band is draw nMC / 10 of the ascending sort, 1-based), got %lld", (long long)nMC); return LPVS_EARGUMENT; }
    if (nMC > kMaxDraws) { set_error("nMC = %lld: the draws of one cell are selected in LDS, at most %lld fit", (long long)nMC, (long long)kMaxDraws); return LPVS_EUNSUPPORTED; }
    if (nb > kMaxBasis) { set_error("nb = %lld: at most %lld basis functions fit next to the draws in LDS", (long long)nb, (long long)kMaxBasis); return LPVS_EUNSUPPORTED; }
    Cn *cn = find_cn(id);
    if (!cn) return LPVS_EARGUMENT;
    if (Nf * nb != cn->n) { set_error("Nf * nb = %lld, the distribution has %lld components", (long long)(Nf * nb), (long long)cn->n); return LPVS_EARGUMENT; }
    LPVS_HIP(hipSetDevice(cn->device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    Events<4> ev;
    for (auto &x : ev.e) LPVS_HIP(hipEventCreate(&x));
    DevBuf Z, out;
    Staged<double> dPhi;
    DrainOnExit drain(sh.s);
    LPVS_TRY(Z.alloc(sizeof(double) * (size_t)nMC * (size_t)cn->n2));
    LPVS_TRY(out.alloc(sizeof(double) * 6 * (size_t)Nf * (size_t)G));
    LPVS_TRY(dPhi.set(Phi_g, G * nb, cn->device, sh.s));
    LPVS_HIP(hipEventRecord(ev.e[0], sh.s));
    LPVS_TRY(sample_device(*cn, nMC, (uint64_t)seed, R, Z.as<double>(), sh.s));
    LPVS_HIP(hipEventRecord(ev.e[1], sh.s));
    int64_t P2 = 16;
    while (P2 < nMC) P2 <<= 1;
    const size_t lds = sizeof(double) * (size_t)(P2 + nb + kBandBlock);
    LPVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cn_bands_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // 1-based nMC / 10 and nMC - nMC / 10 of the ascending sort (src/plotting.jl:91-92)
    cn_bands_kernel<<<(unsigned)(Nf * G), kBandBlock, lds, sh.s>>>(Z.as<double>(), nMC, cn->n, Nf, nb, dPhi.p, G, nMC, P2, phase, nMC / 10 - 1,
                                                                   nMC - nMC / 10 - 1, out.as<double>());
    LPVS_HIP(hipGetLastError());
    LPVS_HIP(hipEventRecord(ev.e[2], sh.s));
    const size_t plane = (size_t)Nf * (size_t)G;
    double *dst[6] = {Fl, Fu, Fm, Pl, Pu, Pm};
    for (int k = 0; k < (phase ? 6 : 3); ++k) LPVS_TRY(out_copy(dst[k], out.as<double>() + k * plane, plane, sh.s));
    float ms0 = 0, ms1 = 0;
    LPVS_HIP(hipEventElapsedTime(&ms0, ev.e[0], ev.e[1]));
    LPVS_HIP(hipEventElapsedTime(&ms1, ev.e[1], ev.e[2]));
    g_timing[1] = ms0; g_timing[2] = ms1; g_timing[3] = (double)ms0 + ms1; g_timing[4] = (double)cn->n2; g_timing[5] = (double)nMC; g_timing[6] = (double)plane;
    return LPVS_OK;
}

}  // namespace
}  // namespace lpvs

using namespace lpvs;

#define LPVS_CN_GUARD(expr)                                                                             \
    try { return (expr); } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }

extern "C" {

int32_t lpvs_cholesky_upper_f64(const double *V, int64_t n2, int32_t device, double *U_out) { LPVS_CN_GUARD(cholesky_impl(V, n2, device, U_out)) }
int32_t lpvs_randn_f64(int64_t seed, int64_t row0, int64_t rows, int64_t cols, int32_t device, double *R_out) {
    LPVS_CN_GUARD(randn_impl(seed, row0, rows, cols, device, R_out))
}
int32_t lpvs_cov_f64(const double *A, int64_t rows, int64_t cols, int32_t device, double *mean_out, double *C_out) {
    LPVS_CN_GUARD(cov_impl(A, rows, cols, device, mean_out, C_out))
}
int32_t lpvs_cn_create_f64(const double *m_re, const double *m_im, const double *V, int64_t n, int32_t device, int64_t *cn) {
    LPVS_CN_GUARD(cn_create_impl(m_re, m_im, V, n, device, cn))
}
int32_t lpvs_cn_destroy(int64_t cn) {
    std::unique_ptr<Cn> gone;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_handles.find(cn);
        if (it == g_handles.end()) return LPVS_OK;
        gone = std::move(it->second);
        g_handles.erase(it);
    }
    (void)hipSetDevice(gone->device);
    return LPVS_OK;
}
int32_t lpvs_cn_rand_f64(int64_t cn, int64_t s, int64_t seed, const double *R, double *Z_re_out, double *Z_im_out) {
    LPVS_CN_GUARD(cn_rand_impl(cn, s, seed, R, Z_re_out, Z_im_out))
}
int32_t lpvs_cn_bands_f64(int64_t cn, int64_t Nf, int64_t nb, const double *Phi_g, int64_t G, int64_t nMC, int64_t seed, const double *R,
                          int32_t phase, double *Fl, double *Fu, double *Fm, double *Pl, double *Pu, double *Pm) {
    LPVS_CN_GUARD(cn_bands_impl(cn, Nf, nb, Phi_g, G, nMC, seed, R, phase, Fl, Fu, Fm, Pl, Pu, Pm))
}
int32_t lpvs_cn_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_timing, 8);
}

}  // extern "C"
