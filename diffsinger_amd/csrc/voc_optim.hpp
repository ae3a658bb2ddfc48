// voc_optim.hpp - the optimisers of the vocoder training rows (include/dsv.h, section "Vocoder optimisers"): one update over a LIST of fp32
// tensors as they lie in memory, and the global gradient norm of such a list with clip_grad_norm_'s coefficient.  Host side: voc_optim_abi.hpp.
//
// TABLES.  A launch gets two tables BY VALUE in its kernel arguments: up to kMtMaxTensors entries (p, g, m, v, n) and up to kMtMaxChunks
// entries (tensor slot, chunk index inside that tensor); workgroup b works on chunk[b] of tensor[b], kMtChunk floats of it (fewer at the
// tensor's end).  Nothing is copied to the device and no buffer has to outlive the call: the argument block is the launch's own.  A list
// that needs more entries than either table holds is split over several launches by the host (voc_optim_abi.hpp); a tensor that does not
// fit the rest of the chunk table continues in the next launch under a new slot.
//   size: 32 * 40 B + 384 * (4 + 1) B = 3200 B of tables, below the 4 KB a kernel argument block holds with room for the scalars and the
//   runtime's hidden arguments.
//
// ADDRESSES.  Any float-aligned pointer works (a view at an odd storage offset).  A chunk starts kMtChunk * k floats behind its tensor's base,
// so it is 16-byte aligned exactly when the base is: a workgroup takes the float4 path when ALL pointers of its tensor are, the scalar path
// otherwise - the same arithmetic on the same values either way.  Element counts and offsets are 64-bit.
//
// ORDER.  No atomics.  The update is element-wise.  The norm: every thread sums the squares of its elements in float32 in ascending order
// (kMtChunk / 256 = 64 terms at most), the workgroup adds its 256 sums in float64 through block_sum's fixed tree and writes ONE float64
// partial at the chunk's GLOBAL index (chunks counted over the whole list, in list order); k_mt_norm_final adds the partials in float64,
// thread t taking t, t + 256, ... in ascending order, then the same tree.  Which launch a chunk ran in does not enter: the result does not
// depend on how the list was split, and two runs are bitwise equal.
#pragma once
#include "fs2_kernels.hpp"
#include "voc_train_common.hpp"

namespace dsd {

constexpr int kMtChunk = 16384;                              // floats per workgroup; a multiple of 4 * 256
constexpr int kMtMaxTensors = 32;
constexpr int kMtMaxChunks = 384;
constexpr int kMtThreads = 256;

struct MtChunks {
    int chunk[kMtMaxChunks];                                 // index of the chunk inside its tensor
    unsigned char tensor[kMtMaxChunks];                      // slot of the tensor table
};

struct MtTensor { float* p; const float* g; float* m; float* v; long long n; };

struct MtStepTable {
    MtTensor t[kMtMaxTensors];
    MtChunks c;
};

struct MtNormTable {
    const float* g[kMtMaxTensors];
    long long n[kMtMaxTensors];
    MtChunks c;
    long long first_chunk;                                   // global index of this launch's chunk 0
};

// ---- the two updates -------------------------------------------------------------------------------------------------------------------------
// RAdam of modules/parallel_wavegan/optimizers/radam.py:57-89 in its order, every product and sum rounded to float32 like the tensor ops it calls:
//   g' = g * gscale ; v = v * b2 + ((1 - b2) g') g' ; m = m * b1 + (1 - b1) g' ; p += (-wd lr) p when wd != 0 ;
//   p += ((-step_size lr) m) / (sqrt(v) + eps) when rectified, p += (-step_size lr) m otherwise
struct MtRAdam {
    const float* gscale;
    float b1, one_minus_b1, b2, one_minus_b2, neg_wd_lr, neg_step_lr, eps;
    int decay, rectified;

    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v, float gs) const {
        g = g * gs;
        v = v * b2 + (one_minus_b2 * g) * g;
        m = m * b1 + one_minus_b1 * g;
        if (decay) p = p + neg_wd_lr * p;
        if (rectified) p = p + (neg_step_lr * m) / (sqrtf(v) + eps);
        else p = p + neg_step_lr * m;
    }
};

// torch.optim.AdamW: adamw_one of fs2_kernels.hpp (the scalars as dsf_adamw_step forms them; the pointers and n of `a` are not used here)
struct MtAdamW {
    AdamWParams a;
    const float* gscale;

    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v, float gs) const { adamw_one(p, g, m, v, a, gs); }
};

template <class Op>
__global__ __launch_bounds__(kMtThreads) void k_mt_step(const MtStepTable tb, const Op op) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const MtTensor t = tb.t[tb.c.tensor[b]];
    const long long off = (long long)tb.c.chunk[b] * kMtChunk;
    const long long rest = t.n - off;
    const int len = rest < kMtChunk ? (int)rest : kMtChunk;
    float* p = t.p + off;
    const float* g = t.g + off;
    float* m = t.m + off;
    float* v = t.v + off;
    const float gs = op.gscale ? op.gscale[0] : 1.f;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
        const int n4 = len >> 2;
        float4* p4 = reinterpret_cast<float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* m4 = reinterpret_cast<float4*>(m);
        float4* v4 = reinterpret_cast<float4*>(v);
#pragma unroll 2
        for (int i = tid; i < n4; i += kMtThreads) {
            float4 pp = p4[i], mm = m4[i], vv = v4[i];
            const float4 gg = g4[i];
            op(pp.x, gg.x, mm.x, vv.x, gs); op(pp.y, gg.y, mm.y, vv.y, gs);
            op(pp.z, gg.z, mm.z, vv.z, gs); op(pp.w, gg.w, mm.w, vv.w, gs);
            p4[i] = pp; m4[i] = mm; v4[i] = vv;
        }
        const int i = (n4 << 2) + tid;                       // the tail of a tensor whose length is no multiple of 4
        if (tid < (len & 3)) {
            float pp = p[i], mm = m[i], vv = v[i];
            op(pp, g[i], mm, vv, gs);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    } else {
        for (int i = tid; i < len; i += kMtThreads) {
            float pp = p[i], mm = m[i], vv = v[i];
            op(pp, g[i], mm, vv, gs);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}

// ---- the global norm ---------------------------------------------------------------------------------------------------------------------------
// Both paths give a thread the SAME elements in the same order (element e of the chunk belongs to thread (e / 4) % 256 on the vector path and
// the scalar path walks e = 4 * (tid + 256 * j) + k likewise), so the alignment of a gradient does not change the sum either.
__global__ __launch_bounds__(kMtThreads) void k_mt_norm_partial(const MtNormTable tb, double* __restrict__ part) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int slot = tb.c.tensor[b];
    const long long off = (long long)tb.c.chunk[b] * kMtChunk;
    const long long rest = tb.n[slot] - off;
    const int len = rest < kMtChunk ? (int)rest : kMtChunk;
    const float* g = tb.g[slot] + off;
    const int n4 = len >> 2;
    float s = 0.f;
    if (((uintptr_t)g & 15) == 0) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 4
        for (int i = tid; i < n4; i += kMtThreads) {
            const float4 x = g4[i];
            s = s + x.x * x.x; s = s + x.y * x.y; s = s + x.z * x.z; s = s + x.w * x.w;
        }
    } else {
        for (int i = tid; i < n4; i += kMtThreads) {
            const float x0 = g[4 * i], x1 = g[4 * i + 1], x2 = g[4 * i + 2], x3 = g[4 * i + 3];
            s = s + x0 * x0; s = s + x1 * x1; s = s + x2 * x2; s = s + x3 * x3;
        }
    }
    if (tid == (n4 & (kMtThreads - 1))) {                    // the tail (< 4 elements) goes to the thread the next float4 would: no thread sums > 64 terms
        for (int i = n4 << 2; i < len; ++i) {
            const float x = g[i];
            s = s + x * x;
        }
    }
    const double tot = block_sum<kMtThreads>((double)s);
    if (tid == 0) part[tb.first_chunk + b] = tot;
}

// out2[0] = sqrt(sum of the partials), out2[1] = min(1, max_norm / (out2[0] + 1e-6)) in float32 (clip_grad_norm_'s coefficient); a NaN stays NaN
__global__ __launch_bounds__(kMtThreads) void k_mt_norm_final(const double* __restrict__ part, long long nparts, float max_norm, float* __restrict__ out2) {
    double s = 0.0;
    for (long long i = threadIdx.x; i < nparts; i += kMtThreads) s += part[i];
    const double tot = block_sum<kMtThreads>(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(tot);
        const float c = __fdiv_rn(max_norm, norm + 1e-6f);
        out2[0] = norm;
        out2[1] = c < 1.f ? c : (c != c ? c : 1.f);
    }
}

}  // namespace dsd
