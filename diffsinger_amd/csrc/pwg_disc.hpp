// pwg_disc.hpp - gfx950 kernels of the ParallelWaveGAN discriminator (modules/parallel_wavegan/models/parallel_wavegan.py:207-300: a stack of
// Conv1d(kernel 3) + LeakyReLU, 1 -> 64 -> ... -> 64 -> 1, dilation 1, 1, 2, ..., layers - 2, 1; configs/tts/pwg.yaml discriminator_params) forward AND
// backward, and the LSGAN criterion it is trained with (modules/hifigan/hifigan.py:337-365).  C ABI in include/dsv.h, section "PWG discriminator";
// host side in pwg_disc_abi.hpp.  Activations are channel-major [B][64][LS] float32, LS = dsv_padded_samples(T), and every kernel leaves [T, LS) at
// zero - the contract of the generator's operators.
//
//   k_pwgd_layer<BWD>   a 64 -> 64 layer, a 128-sample tile of all 64 output channels per workgroup.  The input slab [64][128 + 2 * 8] is
//                       staged ONCE (aligned float4 loads, halo 8 = the largest dilation); the three taps are the same slab read at column offsets
//                       -dil, 0, +dil, i.e. rows tap * 64 + ci of ONE K = 192 contraction on v_mfma_f32_32x32x2_f32 (GemmPipe; the weight stream
//                       is dsv_pack_weight of the [64][192][1] matrix with columns tap * 64 + ci).  Wave w owns row block w & 1 and the two
//                       32-column blocks of tile half w >> 1.
//                         BWD = false:  a = leaky_relu(W x + b)
//                         BWD = true:   G_prev = (W^T * G) m,  m = 1 where the SAVED POST-activation a_prev > 0, else slope (the reference's
//                                       LeakyReLU is inplace: autograd derives the mask from the output, an output of exactly 0 takes the slope);
//                                       the packed matrix is the flipped, transposed one: row ci, column tap * 64 + co = W[co][ci][2 - tap].
//   k_pwgd_wgrad        dW[co][ci][k] = sum_b sum_t G[b][co][t] a_prev[b][ci][t + (k - 1) dil],  db[co] = sum_b sum_t G[b][co][t]: a contraction
//                       over samples.  A workgroup owns the whole 64 x 64 x 3 gradient over one split of kPwgdSplit samples of one batch row
//                       (the form of k_fs_wgrad at half its rows - that kernel's 128-row tile and fixed 16 splits would put the discriminator's
//                       weight gradient on 16 workgroups); partials to a workspace, k_pwgd_wgrad_reduce adds the splits in a fixed order (float64).
//   k_pwgd_first / _last / _first_dx / _last_dgrad / _edge_wgrad / _edge_reduce       the 1 -> 64 and 64 -> 1 layers: plain vector-ALU kernels.
//   k_pwgd_lsgan_partial / _final / _backward        mean((d - c)^2): float64 partial sums in a fixed order (block_sum), a one-workgroup reduction; backward
//                       2 (d - c) / n * g with g read from device memory.
// No atomics, every sum in a fixed order: two calls are bitwise equal.
#pragma once
#include "voc_kernels.hpp"
#include "voc_train_common.hpp"

namespace dsd {

constexpr int kPwgdC = 64;                                   // conv_channels
constexpr int kPwgdTile = 128;                               // samples per workgroup of k_pwgd_layer
constexpr int kPwgdHalo = 8;                                 // largest dilation (layers <= 10)
constexpr int kPwgdLD = kPwgdTile + 2 * kPwgdHalo;           // slab row: 144 floats
constexpr int kPwgdNch = 3 * kPwgdC / 8;                     // 24 chunks of 8 K rows
constexpr int kPwgdSplit = 256;                              // samples per workgroup of k_pwgd_wgrad
constexpr int kPwgdWgFloats = kPwgdC * kPwgdC * 3 + kPwgdC;  // one split's partials: dW then db
constexpr int kPwgdEdgeSplit = 4096;                         // samples per workgroup of k_pwgd_edge_wgrad

struct PwgdLayerParams {
    const float* in;        // [B][64][LS]: x (forward) or G (backward)
    const float4* wp;       // packed [64][192][1]
    const float* bias;      // [64] or nullptr (forward only)
    const float* saved;     // [B][64][LS] post-activation of the layer below, or nullptr: no mask (backward only)
    float* out;             // [B][64][LS]
    int T, LS, dil;
    float slope;
};

// B functor over the slab: chunk kc = tap * 8 + c8 is rows 8 c8 .. 8 c8 + 7 at column offset (tap - 1) * dil
struct PwgdSlabB {
    const float* base; int dil;
    __device__ __forceinline__ const float* operator()(int it, int u) const {
        int kc = 6 * it + u;
        kc = kc < kPwgdNch ? kc : kPwgdNch - 1;
        return base + (kc & 7) * (8 * kPwgdLD) + ((kc >> 3) - 1) * dil;
    }
};

template <bool BWD>
__global__ __launch_bounds__(kThreads, 4) void k_pwgd_layer(const PwgdLayerParams p) {
    __shared__ __attribute__((aligned(16))) float slab[kPwgdC * kPwgdLD];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = w & 1, cb = w >> 1;
    const int t0 = blockIdx.x * kPwgdTile, b = blockIdx.y;
    GemmPipe<1, 2, kPwgdLD, 64, 6, PwgdSlabB> pipe(p.wp + (size_t)rb * kPwgdNch * 64, lane, kPwgdNch,
                                                   PwgdSlabB{slab + 4 * h * kPwgdLD + kPwgdHalo + 64 * cb + j, p.dil});
    pipe.start_a();
    {
        // slab column c holds sample t0 - 8 + c (zero outside [0, T)): 36 aligned float4 per row, all requested before the first LDS write
        const float* xb = p.in + (size_t)b * kPwgdC * p.LS;
        float4 xv[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int idx = tid + 256 * i, row = idx / 36, g = idx - row * 36;
            const int t = t0 - kPwgdHalo + 4 * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t >= 0 && t < p.LS) {
                v = *reinterpret_cast<const float4*>(xb + (size_t)row * p.LS + t);
                v.x = (t + 0 < p.T) ? v.x : 0.f; v.y = (t + 1 < p.T) ? v.y : 0.f; v.z = (t + 2 < p.T) ? v.z : 0.f; v.w = (t + 3 < p.T) ? v.w : 0.f;
            }
            xv[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int idx = tid + 256 * i, row = idx / 36, g = idx - row * 36;
            *reinterpret_cast<float4*>(slab + row * kPwgdLD + 4 * g) = xv[i];
        }
    }
    __syncthreads();
    f32x16 acc[1][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][nb][r] = 0.f;
    pipe.start_b();
    pipe.template run_static<0, kPwgdNch>(acc);
    const size_t rowbase = (size_t)b * kPwgdC * p.LS;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int t = t0 + 64 * cb + 32 * nb + j;
        if (t >= p.LS) continue;
        const bool tv = t < p.T;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 32 * rb + frag_row(r, h);
            const size_t idx = rowbase + (size_t)ch * p.LS + t;
            float v;
            if constexpr (BWD) {
                v = acc[0][nb][r];
                if (p.saved) v = v * (p.saved[idx] > 0.f ? 1.f : p.slope);
            } else {
                v = acc[0][nb][r] + (p.bias ? p.bias[ch] : 0.f);
                v = v > 0.f ? v : v * p.slope;
            }
            p.out[idx] = tv ? v : 0.f;
        }
    }
}

// ---- weight and bias gradient of a 64 -> 64 layer -----------------------------------------------------------------------------------------
constexpr int kPwgdLdg = 33, kPwgdLda = 49;
struct PwgdWgradParams {
    const float* g;         // [B][64][LS] gradient with respect to the layer's pre-activation
    const float* a;         // [B][64][LS] the layer's input (post-activation of the layer below)
    float* part;            // [nsplit][kPwgdWgFloats]
    int T, LS, dil, nch;    // nch = splits per batch row
};

__global__ __launch_bounds__(kThreads, 2) void k_pwgd_wgrad(const PwgdWgradParams p) {
    __shared__ float gt[kPwgdC * kPwgdLdg];
    __shared__ float at[kPwgdC * kPwgdLda];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = w & 1, cb = w >> 1;
    const int split = blockIdx.x, b = split / p.nch, s0 = (split - b * p.nch) * kPwgdSplit;
    const int s1 = min(p.T, s0 + kPwgdSplit);
    const float* gb = p.g + (size_t)b * kPwgdC * p.LS;
    const float* ab = p.a + (size_t)b * kPwgdC * p.LS;
    f32x16 acc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    // thread tid stages G rows (tid >> 3) + 32 q, float4 column tid & 7 [q = 0, 1] and a float4 tid + 256 q [q = 0..2] (12 per row: 8 halo + 32 + 8)
    float4 gv[2], av[3];
    float bsum[2] = {0.f, 0.f};
    auto fetch = [&](int t0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = (tid >> 3) + 32 * q, t = t0 + 4 * (tid & 7);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < p.LS) {
                v = *reinterpret_cast<const float4*>(gb + (size_t)row * p.LS + t);
                v.x = (t + 0 < s1) ? v.x : 0.f; v.y = (t + 1 < s1) ? v.y : 0.f; v.z = (t + 2 < s1) ? v.z : 0.f; v.w = (t + 3 < s1) ? v.w : 0.f;
            }
            gv[q] = v;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int idx = tid + 256 * q, row = idx / 12, g = idx - row * 12;
            const int t = t0 - kPwgdHalo + 4 * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t >= 0 && t < p.LS) {
                v = *reinterpret_cast<const float4*>(ab + (size_t)row * p.LS + t);
                v.x = (t + 0 < p.T) ? v.x : 0.f; v.y = (t + 1 < p.T) ? v.y : 0.f; v.z = (t + 2 < p.T) ? v.z : 0.f; v.w = (t + 3 < p.T) ? v.w : 0.f;
            }
            av[q] = v;
        }
    };
    if (s0 < s1) fetch(s0);
    for (int t0 = s0; t0 < s1; t0 += 32) {
        __syncthreads();                                    // the previous chunk's LDS reads are done
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float* d = gt + ((tid >> 3) + 32 * q) * kPwgdLdg + 4 * (tid & 7);
            d[0] = gv[q].x; d[1] = gv[q].y; d[2] = gv[q].z; d[3] = gv[q].w;
            bsum[q] += (gv[q].x + gv[q].y) + (gv[q].z + gv[q].w);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int idx = tid + 256 * q, row = idx / 12, g = idx - row * 12;
            float* d = at + row * kPwgdLda + 4 * g;
            d[0] = av[q].x; d[1] = av[q].y; d[2] = av[q].z; d[3] = av[q].w;
        }
        __syncthreads();
        if (t0 + 32 < s1) fetch(t0 + 32);
        const float* ap = gt + (32 * rb + j) * kPwgdLdg + h;                           // A[i = co][k = t]: lane half h supplies t = 2 s + h
        const float* bp = at + (32 * cb + j) * kPwgdLda + kPwgdHalo - p.dil + h;       // B[k = t][j = ci], tap 0
#pragma unroll 4
        for (int s2 = 0; s2 < 16; ++s2) {
            const float a = ap[2 * s2];
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = mfma32(a, bp[2 * s2 + k * p.dil], acc[k]);
        }
    }
    float* out = p.part + (size_t)split * kPwgdWgFloats;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = 32 * rb + frag_row(r, h), ci = 32 * cb + j;
            out[(co * kPwgdC + ci) * 3 + k] = acc[k][r];
        }
#pragma unroll
    for (int q = 0; q < 2; ++q) {                           // the 8 threads of a G row sit in consecutive lanes
        float sb = bsum[q];
        sb += __shfl_xor(sb, 1, 64); sb += __shfl_xor(sb, 2, 64); sb += __shfl_xor(sb, 4, 64);
        if ((tid & 7) == 0) out[kPwgdC * kPwgdC * 3 + (tid >> 3) + 32 * q] = sb;
    }
}

// dw [64][64][3] and db [64] (or nullptr): float64 sums, rounded once.  A workgroup owns 64 outputs; its four waves add a quarter of the splits each
// in index order (four times the loads in flight of one walk over all splits), then the quarters are added in order - a fixed order either way.
__global__ __launch_bounds__(256) void k_pwgd_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int nsplit) {
    __shared__ double red[4][64];
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + o;                        // kPwgdWgFloats = 193 * 64: no tail
    const int per = (nsplit + 3) / 4, k0 = q * per, k1 = min(nsplit, k0 + per);
    double s = 0.0;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) s += (double)part[(size_t)k * kPwgdWgFloats + i];
    red[q][o] = s;
    __syncthreads();
    if (q != 0) return;
    s = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
    if (i < kPwgdC * kPwgdC * 3) dw[i] = (float)s;
    else if (db) db[i - kPwgdC * kPwgdC * 3] = (float)s;
}
static_assert(kPwgdWgFloats % 64 == 0, "k_pwgd_wgrad_reduce: 64 outputs per workgroup");

// ---- edge layers --------------------------------------------------------------------------------------------------------------------------
// first layer: a[b][c][t] = leaky_relu(w[c][0] x[t - 1] + w[c][1] x[t] + w[c][2] x[t + 1] + bias[c]);  x [B][LS]
__global__ __launch_bounds__(256) void k_pwgd_first(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                    float* __restrict__ out, int T, int LS, float slope) {
    const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (t >= LS) return;
    float v = 0.f;
    if (t < T) {
        const float* xr = x + (size_t)b * LS;
        const float xm = t > 0 ? xr[t - 1] : 0.f, xp = t + 1 < T ? xr[t + 1] : 0.f;
        v = fmaf(w[3 * c + 2], xp, fmaf(w[3 * c + 1], xr[t], fmaf(w[3 * c], xm, bias ? bias[c] : 0.f)));
        v = v > 0.f ? v : v * slope;
    }
    out[((size_t)b * kPwgdC + c) * LS + t] = v;
}

// last layer: p[b][t] = sum_ci sum_k w[ci][k] a[b][ci][t + k - 1] + bias[0];  ascending ci, then k
__global__ __launch_bounds__(256) void k_pwgd_last(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ out, int T, int LS) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= LS) return;
    float v = 0.f;
    if (t < T) {
        const float* ab = a + (size_t)b * kPwgdC * LS;
        v = bias ? bias[0] : 0.f;
        for (int ci = 0; ci < kPwgdC; ++ci) {
            const float* r = ab + (size_t)ci * LS;
            const float am = t > 0 ? r[t - 1] : 0.f, ap = t + 1 < T ? r[t + 1] : 0.f;
            v = fmaf(w[3 * ci + 2], ap, fmaf(w[3 * ci + 1], r[t], fmaf(w[3 * ci], am, v)));
        }
    }
    out[(size_t)b * LS + t] = v;
}

// data gradient of the last layer: ga[b][ci][t] = (sum_k w[ci][k] gp[b][t - (k - 1)]) m(a[b][ci][t])
__global__ __launch_bounds__(256) void k_pwgd_last_dgrad(const float* __restrict__ gp, const float* __restrict__ a, const float* __restrict__ w,
                                                         float* __restrict__ ga, int T, int LS, float slope) {
    const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (t >= LS) return;
    const size_t idx = ((size_t)b * kPwgdC + c) * LS + t;
    float v = 0.f;
    if (t < T) {
        const float* gr = gp + (size_t)b * LS;
        const float gm = t > 0 ? gr[t - 1] : 0.f, gq = t + 1 < T ? gr[t + 1] : 0.f;
        v = fmaf(w[3 * c], gq, fmaf(w[3 * c + 1], gr[t], w[3 * c + 2] * gm));
        v = v * (a[idx] > 0.f ? 1.f : slope);
    }
    ga[idx] = v;
}

// data gradient of the first layer: dx[b][t] = sum_c sum_k w[c][k] g0[b][c][t - (k - 1)];  ascending c, then k
__global__ __launch_bounds__(256) void k_pwgd_first_dx(const float* __restrict__ g0, const float* __restrict__ w, float* __restrict__ dx, int T, int LS) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= LS) return;
    float v = 0.f;
    if (t < T) {
        const float* gb = g0 + (size_t)b * kPwgdC * LS;
        for (int c = 0; c < kPwgdC; ++c) {
            const float* r = gb + (size_t)c * LS;
            const float gq = t + 1 < T ? r[t + 1] : 0.f, gm = t > 0 ? r[t - 1] : 0.f;
            v = fmaf(w[3 * c + 2], gm, fmaf(w[3 * c + 1], r[t], fmaf(w[3 * c], gq, v)));
        }
    }
    dx[(size_t)b * LS + t] = v;
}

// parameter gradients of both edge layers: part[split][c][k] = sum_t P[t] Q[t + k - 1] (k = 0..2), part[split][c][3] = sum_t P[t] over the split's
// samples of one batch row.  First layer: P = g0[b][c] (cs_p = LS), Q = x[b] (cs_q = 0); last layer: P = gp[b] (cs_p = 0), Q = a[b][c] (cs_q = LS).
// float64 sums: a thread walks its samples in ascending order, then a fixed tree.
__global__ __launch_bounds__(256) void k_pwgd_edge_wgrad(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ part, int T,
                                                         size_t bs_p, size_t cs_p, size_t bs_q, size_t cs_q, int nch) {
    const int tid = threadIdx.x, c = blockIdx.x, split = blockIdx.y, b = split / nch, s0 = (split - b * nch) * kPwgdEdgeSplit;
    const int s1 = min(T, s0 + kPwgdEdgeSplit);
    const float* pr = P + (size_t)b * bs_p + (size_t)c * cs_p;
    const float* qr = Q + (size_t)b * bs_q + (size_t)c * cs_q;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = s0 + tid; t < s1; t += 256) {
        const double pv = (double)pr[t];
        const float qm = t > 0 ? qr[t - 1] : 0.f, qp = t + 1 < T ? qr[t + 1] : 0.f;
        s[0] += pv * (double)qm; s[1] += pv * (double)qr[t]; s[2] += pv * (double)qp; s[3] += pv;
    }
    block_sum(s);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[((size_t)split * kPwgdC + c) * 4 + k] = (float)s[k];
    }
}

// dw [64][3]; db [64] (per_channel_bias) or db [1] = channel 0's sum (the last layer: every channel's workgroups summed the same gp); db may be nullptr
__global__ __launch_bounds__(256) void k_pwgd_edge_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int nsplit,
                                                          int per_channel_bias) {
    const int i = threadIdx.x, c = i >> 2, k = i & 3;
    double s = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) s += (double)part[(size_t)sp * 256 + i];
    if (k < 3) dw[3 * c + k] = (float)s;
    else if (db && (per_channel_bias || c == 0)) db[per_channel_bias ? c : 0] = (float)s;
}

// ---- LSGAN --------------------------------------------------------------------------------------------------------------------------------
constexpr int kPwgdLossThreads = 256, kPwgdLossMaxBlocks = 1024;

__global__ void __launch_bounds__(kPwgdLossThreads) k_pwgd_lsgan_partial(const float* d, float c, double* ws, long long n) {
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * kPwgdLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kPwgdLossThreads) {
        const double e = (double)d[i] - (double)c;
        s += e * e;
    }
    s = block_sum<kPwgdLossThreads>(s);
    if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kPwgdLossThreads) k_pwgd_lsgan_final(const double* ws, float* out, int nblocks, long long n) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kPwgdLossThreads) s += ws[i];
    s = block_sum<kPwgdLossThreads>(s);
    if (threadIdx.x == 0) out[0] = (float)(s / (double)n);
}

__global__ void __launch_bounds__(kPwgdLossThreads) k_pwgd_lsgan_backward(const float* d, float c, const float* g, float* G, long long n) {
    const double sc = 2.0 * (double)g[0] / (double)n;
    for (long long i = (long long)blockIdx.x * kPwgdLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kPwgdLossThreads)
        G[i] = (float)(((double)d[i] - (double)c) * sc);
}

}  // namespace dsd
