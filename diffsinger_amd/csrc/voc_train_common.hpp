// voc_train_common.hpp - the device pieces the vocoder-training kernels share (pwg_disc.hpp, pwg_train.hpp, hifigan_train.hpp,
// voc_stft_loss.hpp): the fixed-order workgroup sum (block_sum.hpp, shared with the objectives), the split length and tile stride of the
// split-K weight gradients and the reduction of their splits.  Every "two calls are bitwise equal" claim of those headers rests on the
// orders written down there and HERE, once.  Host-side checks: voc_train_host.hpp.
#pragma once
#include "block_sum.hpp"

namespace dsd {

// ---- split-K weight gradients (k_pwgt_wgrad, k_hgt_wgrad) ---------------------------------------------------------------------------------------
constexpr int kSplitK = 512;                                 // samples per workgroup
constexpr int kSplitLdw = 33;                                // LDS row stride of the 128 x 32 and 64 x 32 tiles

// out[i] = sum_k part[k * n + i] in float64, ascending k, rounded once: the splits of a weight gradient
__global__ __launch_bounds__(256) void k_split_reduce(const float* __restrict__ part, float* __restrict__ out, int n, int nsplit) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < nsplit; ++k) s += (double)part[(size_t)k * n + i];
    out[i] = (float)s;
}

}  // namespace dsd
