// fold_device.h -- the device pieces the folding kernels share (bls.hip, fold.hip): the phase bin of the exact product, the inclusive
// prefix sums of a histogram row by one wave, and the sum over a wrapping run of bins from them.
#pragma once

#include <hip/hip_runtime.h>

namespace lpvs {

// the phase bin of (f, t): the fractional part of the exact product f t
__device__ inline int bls_bin(double f, double t, int nbins, double dnbins) {
    const double p = f * t, e = fma(f, t, -p);
    double phi = (p - rint(p)) + e;
    if (phi < 0.0) phi = phi + 1.0;
    const int b = (int)floor(phi * dnbins);
    return b < 0 ? 0 : b < nbins - 1 ? b : nbins - 1;                      // (b < 0: only when f t overflows and phi is not a number)
}

// the sum over the bins b .. b + k - 1 (wrapping) of a row from its inclusive prefix sums I: before = I[b - 1] (0 for b = 0), total = I[nb - 1]
template <typename T>
__device__ inline T bls_box(const T *I, int nb, int b, int k, T before, T total) {
    const int e = b + k;
    return e <= nb ? I[e - 1] - before : (total - before) + I[e - nb - 1];
}

// inclusive prefix sums of a row in place, by one wave: lane l owns the bins l chunk .. (l + 1) chunk - 1
template <typename T>
__device__ inline void bls_prefix_row(T *H, int nb, int lane) {
    const int chunk = (nb + 63) / 64, lo = lane * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    T sum = 0;
    for (int i = lo; i < hi; ++i) sum += H[i];
    T incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    T run = incl - sum;
    for (int i = lo; i < hi; ++i) { run += H[i]; H[i] = run; }
}

}  // namespace lpvs
