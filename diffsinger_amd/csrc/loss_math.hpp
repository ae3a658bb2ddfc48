// loss_math.hpp - the scalar pieces the objectives share (fs2_loss.hpp, fs2_cwt.hpp, pe_train.hpp, k_fs_l1_bwd), over float and double: the
// overloaded device functions resolve by T (expf / log1pf under float, exp / log1p under double), so a kernel keeps its arithmetic type.
#pragma once
#include "dsd_kernels.hpp"

namespace dsd {

// torch.sign: 0 at 0, NaN stays NaN
template <typename T>
__device__ __forceinline__ T loss_sign(T d) { return d > T(0) ? T(1) : (d < T(0) ? T(-1) : d); }

// F.binary_cross_entropy_with_logits(x, z) of one element: max(x, 0) - x z + log1p(exp(-|x|))
template <typename T>
__device__ __forceinline__ T bce_logits(T x, T z) { return fmax(x, T(0)) - x * z + log1p(exp(-fabs(x))); }

// its derivative with respect to x: sigmoid(x) - z, the sigmoid from exp(-|x|) (no overflow on either side)
template <typename T>
__device__ __forceinline__ T bce_logits_grad(T x, T z) {
    const T e = exp(-fabs(x));
    return (x >= T(0) ? T(1) / (T(1) + e) : e / (T(1) + e)) - z;
}

}  // namespace dsd
