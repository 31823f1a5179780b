// nufft_coord.h -- where a sample sits on the fine grid of the non-uniform FFTs, shared by the type-1 spreading (nufft.hip) and the
// type-2 interpolation (eval.hip): the phase D x reduced to turns in double-double, the grid position, and the kernel values.
// Device code; every product is rounded separately (the files that include it are built with -ffp-contract=off) and the fused
// multiply-adds are written out.
#pragma once
#include <hip/hip_runtime.h>

#include "nufft_bins.h"

namespace lpvs {

constexpr double kNuBeta = 2.30 * kNuWidth;   // phi(z) = exp(beta (sqrt(1 - z^2) - 1))

// (D_hi + D_lo) x in turns, reduced to [0, 1): the product with an FMA-exact low part, times 1 / (2 pi) in double-double -- the phase of
// the REAL product, not of its rounding
__device__ inline double nu_phase_turns(double D_hi, double D_lo, double xv) {
    constexpr double I2PI_HI = 0.15915494309189535, I2PI_LO = -9.8393384885635288e-18;   // 1 / (2 pi) in double-double
    const double th = D_hi * xv, tl = fma(D_hi, xv, -th) + D_lo * xv;                     // D x (double-double)
    const double uh = th * I2PI_HI, ul = fma(th, I2PI_HI, -uh) + (th * I2PI_LO + tl * I2PI_HI);   // turns
    double r = (uh - rint(uh)) + ul;
    r -= floor(r);                                   // [0, 1)
    return r;
}
// position p in [0, nf) of r turns; *g0: grid points g0 .. g0 + 15 lie within |g - p| <= 8 (g0 may be negative: wrap it)
__device__ inline double nu_grid_pos(double r, int nf, int *g0) {
    double p = r * (double)nf;
    if (p >= (double)nf) p -= (double)nf;
    *g0 = (int)ceil(p - 0.5 * kNuWidth);
    return p;
}
// kernel value of grid point g0 + k for a sample at p
__device__ inline double nu_tap(int g0, int k, double p) {
    const double z = ((double)(g0 + k) - p) * (2.0 / kNuWidth);
    const double s = 1.0 - z * z;
    return s > 0.0 ? exp(kNuBeta * (sqrt(s) - 1.0)) : exp(-kNuBeta);
}

}  // namespace lpvs
