// basis_device.h -- one basis function's activation, shared by the table kernel (basis.hip) and model evaluation (eval.hip).
// Device code; every product is rounded separately, in the reference's order (src/lsfft.jl:195, 202).
#pragma once
#include <hip/hip_runtime.h>

namespace lpvs {

__device__ inline double basis_sgn(double x) { return (double)((x > 0) - (x < 0)); }

// exp((-gamma) (v - c)^2), times [sign v == sign c] with coulomb
__device__ inline double basis_activation(double v, double c, double gamma, int coulomb) {
    const double d = v - c;
    double k = exp(-gamma * (d * d));
    if (coulomb) k = k * (basis_sgn(v) == basis_sgn(c) ? 1.0 : 0.0);  // src/lsfft.jl:202
    return k;
}

}  // namespace lpvs
