// lomb_device.h -- the device functions the Lomb-Scargle kernels share (lomb.hip: lombscargle and its windowed twins; lomb_boot.hip: the
// bootstrap): the phase of an exact product, the fixed-order sums over a workgroup, over the four sample lanes and over slabs, and the
// closed-form fit of one (frequency, signal).
#pragma once
#include "lpvs_internal.h"
#include "lomb_plan.h"

namespace lpvs {

constexpr int LB_TF = kLombFreqTile, LB_LANES = kLombSampleLanes, LB_STAGE = kLombStage;
static_assert(LB_TF * LB_LANES == 256 && LB_STAGE == 256 && kLombSumBlock == 256, "the kernels are written for 256 threads");

// sum over the workgroup's 256 threads in a pairwise tree (every thread calls it)
__device__ inline double lomb_block_sum(double v, double *red) {
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

// cos, sin of 2 pi f t from the exact product
__device__ inline void lomb_sincos(double f, double t, double *sn, double *cs) {
    const double p = f * t, e = fma(f, t, -p);
    const double r = (p - rint(p)) + e;               // turns in [-1/2, 1/2] (+ e); p - rint(p) is exact
    sincospi(2.0 * r, sn, cs);
}

// the four sample lanes of one accumulator, added as (0 + 1) + (2 + 3)
__device__ inline double lomb_lane_sum(const double (*red)[LB_TF], int fl) { return (red[0][fl] + red[1][fl]) + (red[2][fl] + red[3][fl]); }

// sums[e] = pairwise tree over the slabs of part[slab][e], e < nrow Nf: slabs 2i and 2i + 1 first, then pairs of pairs, ... (a binary
// counter of partial sums), what is left over added from the smallest piece up
__device__ inline double lomb_pairwise(const double *__restrict__ p, int64_t stride, int64_t n) {
    double stack[12];                                                      // n <= kLombMaxSlabs = 2^10
    for (int64_t i = 0; i < n; ++i) {
        double v = p[i * stride];
        int b = 0;
        for (; (i >> b) & 1; ++b) v = stack[b] + v;
        stack[b] = v;
    }
    double r = 0.0;
    bool have = false;
    for (int b = 0; b < 12; ++b)
        if ((n >> b) & 1) { r = have ? stack[b] + r : stack[b]; have = true; }
    return r;
}

// CONSTANT SIGNALS.  The standard power is 0 when YY is within rounding of 0 (lomb_yy_noise of lomb_plan.h), not only when it is exactly 0:
// a constant signal with unequal weights leaves a YY that is a rounding residue, and p / YY would be a quotient of two noise terms.
struct LombFit { double pw, a, b, c; bool degenerate; };
// the fit of one (frequency, signal) from its sums: R = sum w y^2 of the signal as given, removed = the mean that centring took out
__device__ inline LombFit lomb_fit(double C, double S, double C2, double S2, double YC, double YS, double Y, double YY, double R, double removed, int fit_mean,
                                   int center, int psd, double Nsamples) {
    const double yy_noise = lomb_yy_noise(Nsamples, center != 0, fit_mean != 0, R, YY);
    double CC = 0.5 * (1.0 + C2), SS = 0.5 * (1.0 - C2), CS = 0.5 * S2;
    const double scale = CC + SS;
    if (fit_mean) {
        YY = fma(-Y, Y, YY); YC = fma(-Y, C, YC); YS = fma(-Y, S, YS);
        CC = fma(-C, C, CC); SS = fma(-S, S, SS); CS = fma(-C, S, CS);
    }
    const double D = fma(CC, SS, -(CS * CS));
    LombFit r = {0.0, 0.0, 0.0, removed + (fit_mean ? Y : 0.0), false};
    if (!(D > kLombDegenerate * (scale * scale))) {
        r.degenerate = true;
        r.c = 0.0;
    } else {
        const double p = (fma(SS * YC, YC, (CC * YS) * YS) - 2.0 * ((CS * YC) * YS)) / D;
        r.a = fma(SS, YC, -(CS * YS)) / D;
        r.b = fma(CC, YS, -(CS * YC)) / D;
        if (fit_mean) r.c = removed + ((Y - r.a * C) - r.b * S);
        r.pw = psd ? p * (0.5 * Nsamples) : (YY > yy_noise ? p / YY : 0.0);
    }
    return r;
}

}  // namespace lpvs
