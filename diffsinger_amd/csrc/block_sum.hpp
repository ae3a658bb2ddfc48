// block_sum.hpp - the fixed-order workgroup sum of every training kernel: the vocoder's (voc_train_common.hpp and its users) and the
// objectives' (fs2_loss.hpp, fs2_cwt.hpp, the f0 loss of pe_train.hpp, k_fs_l1_* of fs2_kernels.hpp).  Every "two calls are bitwise equal"
// claim of those headers rests on the order written down HERE, once.
#pragma once
#include "dsd_kernels.hpp"

namespace dsd {

// v[k] = sum over the workgroup's THREADS threads of v[k], N values of T (float or double) at a time: a tree of strides THREADS / 2, ..., 1
// (thread i adds thread i + stride), a barrier after each level; each v[k] goes through the tree on its own, so batching N sums into one
// call changes no bit of any of them.  Every thread holds the totals: the last barrier is behind the last level.
//
// The reuse rule.  The array is one static allocation per instantiation, nothing waits in front of the first stores and nothing behind the
// final reads of red[k][0].  So:
//   - a kernel's FIRST sum is block_sum: nobody has touched the array yet;
//   - every LATER sum of the kernel (a dependent one: mean, then variance) is block_sum_again: a barrier, then block_sum.  That barrier is
//     enough: a thread passes it only after every thread has read red[k][0] of the sum before, and nobody writes the array sooner;
//   - calls of different instantiations (N, THREADS, T) in one kernel own separate static arrays and ADD to the kernel's LDS:
//     N * THREADS * sizeof(T) bytes each.  Independent sums belong in one call.
template <int N, int THREADS = 256, typename T>
__device__ __forceinline__ void block_sum(T (&v)[N]) {
    __shared__ T red[N][THREADS];
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

template <int THREADS = 256, typename T>
__device__ __forceinline__ T block_sum(T a) {
    T v[1] = {a};
    block_sum<1, THREADS>(v);
    return v[0];
}

template <int N, int THREADS = 256, typename T>
__device__ __forceinline__ void block_sum_again(T (&v)[N]) {
    __syncthreads();
    block_sum<N, THREADS>(v);
}

template <int THREADS = 256, typename T>
__device__ __forceinline__ T block_sum_again(T a) {
    __syncthreads();
    return block_sum<THREADS>(a);
}

}  // namespace dsd
