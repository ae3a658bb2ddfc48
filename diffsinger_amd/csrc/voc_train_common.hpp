// voc_train_common.hpp - the device pieces the vocoder-training kernels share (pwg_disc.hpp, pwg_train.hpp, hifigan_train.hpp,
// voc_stft_loss.hpp): the fixed-order workgroup sum, the split length and tile stride of the split-K weight gradients and the reduction of
// their splits.  Every "two calls are bitwise equal" claim of those headers rests on the orders written down HERE, once.  Host-side checks:
// voc_train_host.hpp.
#pragma once
#include "dsd_kernels.hpp"

namespace dsd {

// ---- fixed-order workgroup sum --------------------------------------------------------------------------------------------------------------
// v[k] = sum over the workgroup's THREADS threads of v[k], N float64 values at a time: a tree of strides THREADS / 2, ..., 1 (thread i adds
// thread i + stride), a barrier after each level.  Thread 0 holds the totals (every thread does: the last barrier is behind the last level).
// AT MOST ONE CALL PER KERNEL: the array is one static allocation per instantiation and nothing waits behind the final reads.
template <int N, int THREADS = 256>
__device__ __forceinline__ void block_sum(double (&v)[N]) {
    __shared__ double red[N][THREADS];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int st = THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int k = 0; k < N; ++k) red[k][tid] += red[k][tid + st];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = red[k][0];
}

template <int THREADS = 256>
__device__ __forceinline__ double block_sum(double a) {
    double v[1] = {a};
    block_sum<1, THREADS>(v);
    return v[0];
}

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
