// fs2_dropout.hpp - counter-based training dropout of FastSpeech2 (C ABI in include/dsf.h: dsf_dropout, dsf_dropout_add_keep,
// dsf_dropout_add_keep_bwd); included at the end of dsd.hip (one translation unit: shares fail(), HIP_TRY).
//
// The mask is a pure function of (seed, step, site, element): for the flat fp32 index i of a buffer, q = i >> 2, j = i & 3,
//     w = Philox4x32-10(counter = (q lo32, q hi32, site, step lo32), key = (seed lo32, seed hi32))[j],   element i is KEPT iff w >= thr
// (unsigned 32-bit compare; thr = min(round(p * 2^32), 2^32 - 1) and scale = (float)(1 / (1 - p)) are formed by the host).  One Philox call
// serves the four elements of a float4, so the backward regenerates the mask instead of reading a saved one and a test restates it on the
// CPU (oracle/philox_oracle.py holds the same generator; the round function is philox_normal's, dsd_kernels.hpp, restated here so that the
// sampler's kernels stay untouched).  seed and step live in a DEVICE cell (state[0], state[1]): a captured training step stays valid when
// the step advances.
//
// Every kernel is a grid-stride loop over float4 quads with 64-bit indices; when a base address is not 16-byte aligned (a view that starts
// inside its storage) the same kernel runs one element per thread and step, every element drawing word j of its own quad: the mask is that
// of the view's own flat indices on either path.  Plain vector stores only, no atomics, fixed arithmetic (__fmul_rn / __fadd_rn: no
// contraction), so two launches are bitwise equal and the host restatement is exact.
#pragma once

namespace dsd {

constexpr int kDropThreads = 256;
constexpr int kDropMaxBlocks = 2048;       // 8 workgroups of 256 threads on each of 256 CUs: one resident pass, then the grid strides

struct FsDropKey {
    unsigned k0, k1, site, step;
};

__device__ __forceinline__ FsDropKey drop_key(const unsigned long long* state, unsigned site) {
    const unsigned long long seed = state[0], step = state[1];
    return FsDropKey{(unsigned)seed, (unsigned)(seed >> 32), site, (unsigned)step};
}

// the four output words of Philox4x32-10 for quad q
__device__ __forceinline__ uint4 drop_words(const FsDropKey& key, unsigned long long q) {
    unsigned c0 = (unsigned)q, c1 = (unsigned)(q >> 32), c2 = key.site, c3 = key.step;
    unsigned k0 = key.k0, k1 = key.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ unsigned drop_word(const FsDropKey& key, long long i) {
    const uint4 w = drop_words(key, (unsigned long long)i >> 2);
    const int j = (int)(i & 3);
    return j == 0 ? w.x : j == 1 ? w.y : j == 2 ? w.z : w.w;
}

__device__ __forceinline__ float drop_apply(float x, unsigned w, unsigned thr, float scale) { return w >= thr ? __fmul_rn(x, scale) : 0.0f; }

struct FsDropParams {
    const float* x;
    float* y;
    long long n;
    const unsigned long long* state;
    unsigned site, thr;
    float scale;
};

// y[i] = kept(i) ? x[i] * scale : 0.  VEC: x and y are 16-byte aligned - float4 quads, then the n & 3 elements behind the last whole quad.
template <bool VEC>
__global__ void __launch_bounds__(kDropThreads) k_fs_dropout(FsDropParams p) {
    const FsDropKey key = drop_key(p.state, p.site);
    const long long gid = (long long)blockIdx.x * kDropThreads + threadIdx.x, stride = (long long)gridDim.x * kDropThreads;
    if constexpr (VEC) {
        const long long n4 = p.n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(p.x);
        float4* y4 = reinterpret_cast<float4*>(p.y);
        for (long long q = gid; q < n4; q += stride) {
            const uint4 w = drop_words(key, (unsigned long long)q);
            const float4 v = x4[q];
            y4[q] = make_float4(drop_apply(v.x, w.x, p.thr, p.scale), drop_apply(v.y, w.y, p.thr, p.scale), drop_apply(v.z, w.z, p.thr, p.scale),
                                drop_apply(v.w, w.w, p.thr, p.scale));
        }
        const long long i = (n4 << 2) + gid;                        // the tail: at most three elements, threads 0..2 of the grid
        if (gid < (p.n & 3)) p.y[i] = drop_apply(p.x[i], drop_word(key, i), p.thr, p.scale);
    } else {
        for (long long i = gid; i < p.n; i += stride) p.y[i] = drop_apply(p.x[i], drop_word(key, i), p.thr, p.scale);
    }
}

struct FsDropAddParams {
    const float* x;         // forward: the branch that is dropped [B][C][TS];  backward: dy
    const float* res;       // forward: the residual [B][C][TS];                backward: unused
    const float* keep;      // [B][T] 0 / 1, or null (all ones)
    float* y;               // forward: y;                                      backward: dx
    float* dres;            // backward only, or null
    unsigned per_b;         // C * TS, the elements of one batch item (below 2^31)
    int T, TS;
    const unsigned long long* state;
    unsigned site, thr;
    float scale;
};

// forward, element (b, c, t):  y = t < T ? keep[b][t] * (res + (kept ? x * scale : 0)) : 0
// backward:                    dres = t < T ? dy * keep[b][t] : 0,  dx = kept ? dres * scale : 0
template <bool BWD>
__device__ __forceinline__ float drop_add_elem(const FsDropAddParams& p, const float* keep_row, int t, unsigned w, float x, float r, float* dres) {
    if (t >= p.T) {
        if (BWD) *dres = 0.0f;
        return 0.0f;
    }
    const float k = keep_row ? keep_row[t] : 1.0f;
    if constexpr (BWD) {
        const float g = __fmul_rn(x, k);
        *dres = g;
        return drop_apply(g, w, p.thr, p.scale);
    } else {
        return __fmul_rn(k, __fadd_rn(r, drop_apply(x, w, p.thr, p.scale)));
    }
}

// grid (x, B): workgroups (., b) stride over the elements of batch item b - the batch index costs no division and the frame index one 32-bit
// remainder; the Philox counter is the element's flat index in the whole [B][C][TS] buffer
template <bool BWD, bool VEC>
__global__ void __launch_bounds__(kDropThreads) k_fs_dropout_add_keep(FsDropAddParams p) {
    const FsDropKey key = drop_key(p.state, p.site);
    const unsigned gid = blockIdx.x * kDropThreads + threadIdx.x, stride = gridDim.x * kDropThreads;
    const long long base = (long long)blockIdx.y * p.per_b;
    const float* keep_row = p.keep ? p.keep + (long long)blockIdx.y * p.T : nullptr;
    if constexpr (VEC) {
        const unsigned n4 = p.per_b >> 2, ts4 = (unsigned)p.TS >> 2;      // TS is a multiple of 32: a quad never crosses a row
        const float4* x4 = reinterpret_cast<const float4*>(p.x + base);
        const float4* r4 = BWD ? nullptr : reinterpret_cast<const float4*>(p.res + base);
        float4* y4 = reinterpret_cast<float4*>(p.y + base);
        float4* d4 = p.dres ? reinterpret_cast<float4*>(p.dres + base) : nullptr;
        for (unsigned q = gid; q < n4; q += stride) {
            const int t = (int)((q % ts4) << 2);
            const uint4 w = drop_words(key, (unsigned long long)(base >> 2) + q);
            const float4 v = x4[q];
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f), g = r, o;
            if constexpr (!BWD) r = r4[q];
            o.x = drop_add_elem<BWD>(p, keep_row, t, w.x, v.x, r.x, &g.x);
            o.y = drop_add_elem<BWD>(p, keep_row, t + 1, w.y, v.y, r.y, &g.y);
            o.z = drop_add_elem<BWD>(p, keep_row, t + 2, w.z, v.z, r.z, &g.z);
            o.w = drop_add_elem<BWD>(p, keep_row, t + 3, w.w, v.w, r.w, &g.w);
            y4[q] = o;
            if constexpr (BWD) if (d4) d4[q] = g;
        }
    } else {
        for (unsigned e = gid; e < p.per_b; e += stride) {
            const long long i = base + e;
            float g = 0.0f;
            float r = 0.0f;
            if constexpr (!BWD) r = p.res[i];
            const float o = drop_add_elem<BWD>(p, keep_row, (int)(e % (unsigned)p.TS), drop_word(key, i), p.x[i], r, &g);
            p.y[i] = o;
            if constexpr (BWD) if (p.dres) p.dres[i] = g;
        }
    }
}

static inline unsigned drop_grid(long long work) { return (unsigned)std::min<long long>((work + kDropThreads - 1) / kDropThreads, kDropMaxBlocks); }

}  // namespace dsd

extern "C" int64_t dsf_dropout_grid_elements(void) { return (int64_t)kDropMaxBlocks * kDropThreads * 4; }

extern "C" int dsf_dropout(const float* x, float* y, int64_t n, const uint64_t* state, uint32_t site, uint32_t thr, float scale, void* stream) {
    if (!x || !y || !state) return fail(DSD_ERR_INVALID, "dsf_dropout: null argument");
    if (n < 1) return fail(DSD_ERR_INVALID, "dsf_dropout: n must be positive (got %lld)", (long long)n);
    if (thr == 0) return fail(DSD_ERR_INVALID, "dsf_dropout: thr == 0 drops nothing (p must lie in (0, 1); the caller bypasses the op at p == 0)");
    FsDropParams p{x, y, (long long)n, (const unsigned long long*)state, site, thr, scale};
    if ((((uintptr_t)x | (uintptr_t)y) & 15) == 0)
        hipLaunchKernelGGL((k_fs_dropout<true>), dim3(drop_grid(std::max<long long>(n >> 2, 1))), dim3(kDropThreads), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((k_fs_dropout<false>), dim3(drop_grid(n)), dim3(kDropThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

static int drop_add_launch(const char* who, bool bwd, const float* x, const float* res, const float* keep, float* y, float* dres, int32_t B, int32_t C,
                           int32_t T, const uint64_t* state, uint32_t site, uint32_t thr, float scale, void* stream) {
    if (!x || !y || !state || (!bwd && !res)) return fail(DSD_ERR_INVALID, "%s: null argument", who);
    if (B < 1 || C < 1 || T < 1) return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d C=%d T=%d)", who, B, C, T);
    if (thr == 0) return fail(DSD_ERR_INVALID, "%s: thr == 0 drops nothing (p must lie in (0, 1); the caller bypasses the op at p == 0)", who);
    const long long per_b = (long long)C * ((T + 31) / 32 * 32);
    if (B > 65535 || per_b > 0x7fffffffLL)
        return fail(DSD_ERR_INVALID, "%s: B=%d above 65535 or C * padded_frames(T) = %lld above 2^31 - 1: split the batch", who, B, per_b);
    FsDropAddParams p{};
    p.x = x; p.res = res; p.keep = keep; p.y = y; p.dres = dres;
    p.T = T; p.TS = (T + 31) / 32 * 32; p.per_b = (unsigned)per_b;
    p.state = (const unsigned long long*)state; p.site = site; p.thr = thr; p.scale = scale;
    const bool vec = (((uintptr_t)x | (uintptr_t)res | (uintptr_t)y | (uintptr_t)dres) & 15) == 0;
    // about kDropMaxBlocks workgroups in all, one at least per batch item
    const long long work = vec ? per_b >> 2 : per_b;
    const unsigned gx = (unsigned)std::min<long long>((work + kDropThreads - 1) / kDropThreads, std::max(1, kDropMaxBlocks / B));
    const dim3 grid(gx, (unsigned)B), blk(kDropThreads);
    hipStream_t s = (hipStream_t)stream;
    if (bwd) {
        if (vec) hipLaunchKernelGGL((k_fs_dropout_add_keep<true, true>), grid, blk, 0, s, p);
        else hipLaunchKernelGGL((k_fs_dropout_add_keep<true, false>), grid, blk, 0, s, p);
    } else {
        if (vec) hipLaunchKernelGGL((k_fs_dropout_add_keep<false, true>), grid, blk, 0, s, p);
        else hipLaunchKernelGGL((k_fs_dropout_add_keep<false, false>), grid, blk, 0, s, p);
    }
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_dropout_add_keep(const float* x, const float* res, const float* keep, float* y, int32_t B, int32_t C, int32_t T, const uint64_t* state,
                                    uint32_t site, uint32_t thr, float scale, void* stream) {
    return drop_add_launch("dsf_dropout_add_keep", false, x, res, keep, y, nullptr, B, C, T, state, site, thr, scale, stream);
}

extern "C" int dsf_dropout_add_keep_bwd(const float* dy, const float* keep, float* dx, float* dres, int32_t B, int32_t C, int32_t T, const uint64_t* state,
                                        uint32_t site, uint32_t thr, float scale, void* stream) {
    return drop_add_launch("dsf_dropout_add_keep_bwd", true, dy, nullptr, keep, dx, dres, B, C, T, state, site, thr, scale, stream);
}
