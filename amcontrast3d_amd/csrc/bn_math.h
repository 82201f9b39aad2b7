// Training-mode BatchNorm's arithmetic, once: every kernel that finishes statistics or normalises a value (bn.hip,
// sa_tail.hip, lagg.hip) calls these three, and tests/bn_ref.py restates them operation by operation.  The library is built
// without floating-point contraction, so the expressions below are evaluated as written; do not reorder them.
#pragma once
#include "common.h"

namespace amc {

// {sum x, sum x^2} over `cnt` values -> mean, invstd = 1 / sqrt(biased variance + eps), and the unbiased variance that
// nn.BatchNorm keeps as running_var.  fp64 throughout, rounded to float once at the end.
__device__ __forceinline__ void bn_moments(double s1, double s2, double cnt, float eps, float &mean, float &invstd,
                                           float &var_unbiased)
{
    const double mu = s1 / cnt;
    double var = s2 / cnt - mu * mu;
    if (var < 0.0) var = 0.0;
    mean = (float)mu;
    invstd = (float)(1.0 / sqrt(var + (double)eps));
    var_unbiased = (float)(cnt > 1.0 ? var * cnt / (cnt - 1.0) : var);
}

// nn.BatchNorm's exponential buffer update of channel c: running.mul_(1 - m).add_(batch, alpha=m), and the counter once per
// layer (at c == 0).  momentum < 0 stands for None (cumulative average): bn_running_kernel's job, nothing here.
__device__ __forceinline__ void bn_running_update(int c, float momentum, float mean, float var_unbiased, float *running_mean,
                                                  float *running_var, long long *tracked)
{
    if (running_mean && momentum >= 0.f) {
        running_mean[c] = running_mean[c] * (1.f - momentum) + momentum * mean;
        running_var[c] = running_var[c] * (1.f - momentum) + momentum * var_unbiased;
        if (c == 0 && tracked) *tracked += 1;
    }
}

// ((x - mean) * invstd) * gamma + beta, four rounded float operations in PyTorch's order
__device__ __forceinline__ float bn_val(float x, float mean, float invstd, float gamma, float beta)
{
    return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(x, mean), invstd), gamma), beta);
}

}  // namespace amc
