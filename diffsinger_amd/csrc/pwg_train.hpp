// pwg_train.hpp - gfx950 kernels of ParallelWaveGAN GENERATOR TRAINING: the training forward of a gated residual block (k_pwg_layer's arithmetic
// plus the saved gate pre-activations) and the backward of every piece of the generator (modules/parallel_wavegan/models/parallel_wavegan.py:21-177,
// layers/residual_block.py:96-129, layers/upsample.py:63-183).  C ABI in include/dsv.h, section "PWG generator training"; host side in
// pwg_train_abi.hpp.  Activations are channel-major [B][C][LS] float32, LS = dsv_padded_samples(L); every kernel leaves [L, LS) at zero.
//
// Saved per block: its input x_l [B][64][LS] (the weight gradient needs it anyway) and the gate pre-activations a_l [B][128][LS]; the backward
// recomputes tanh, sigmoid and z from a_l with the forward's formula (hardware exponential).  With s = sqrt(0.5), dx' the gradient at the block's
// residual output and dS the gradient at the skip sum (the same tensor for every block):
//
//   k_pwgt_layer      k_pwg_layer + the store of a_l: the same staging, the same two contractions in the same order, the same gate.
//   k_pwgt_gate_bwd   dz = W_skip^T dS + W_out^T (s dx')  (K = 128 -> 64 rows; the two K halves on two wave pairs, added through LDS in a fixed
//                     order), then da_tanh = dz sigmoid(g) (1 - tanh(a)^2), da_sig = dz tanh(a) sigmoid(g) (1 - sigmoid(g)) -> da [B][128][LS].
//                     The last block's residual output is never read: dx' = nullptr, only the skip half runs.
//   k_pwgt_conv_bwd   dx = s dx' + sum_tap W_conv[:, :, tap]^T da(t - (tap - 1) d): the forward's "taps are rows of one staged tile" with three
//                     da tiles fetched at their own offsets (K = 384 -> 64 rows, again two K halves), and from the centre tile the running
//                     conditioning gradient dC (+)= W_aux^T da (K = 128 -> aux rows) with a `first` flag like the forward's skip sum.
//   k_pwgt_wgrad      dW [128][N] = sum_t P(t) Q(t)^T and db = sum_t P over one split of kSplitK samples of one batch row and one group of
//                     64 columns per workgroup (the tile k_hgt_wgrad runs too); k_split_reduce (voc_train_common.hpp) adds the splits in index
//                     order in float64.
//                       block conv + aux:   P = da,            Q = [x(t - d); x(t); x(t + d); c(t)]     N = 192 + aux
//                       block out + skip:   P = [s dx'; dS],   Q = z(t) recomputed from a_l              N = 64
//                       last_conv_layers[1]: P = [g; 0],       Q = relu(saved)                           N = 64
//   k_pwgt_rowdot / _last_dgrad / _relu_mask / _up_dgrad / _up_wgrad / _up_wreduce / _convin_wgrad
//                     the 1-channel, vector-shaped and frame-rate pieces: plain vector-ALU kernels, float64 sums in a fixed order.
// No atomics; every sum runs in a fixed order: two calls are bitwise equal.
#pragma once
#include "pwg_kernels.hpp"
#include "voc_train_common.hpp"

namespace dsd {

// tanh(a) and sigmoid(g) exactly as k_pwg_layer evaluates them
__device__ __forceinline__ float pwgt_tanh(float xa) { return 1.f - 2.f / (__expf(2.f * xa) + 1.f); }
__device__ __forceinline__ float pwgt_sigmoid(float xg) { return 1.f / (1.f + __expf(-xg)); }

// ---- training forward of a block ------------------------------------------------------------------------------------------------------------
struct PwgtLayerParams {
    PwgLayerParams f;
    float* a_out;           // [B][128][LS] gate pre-activations (bias included), zero in [L, LS)
};

__global__ __launch_bounds__(kThreads, 4) void k_pwgt_layer(const PwgtLayerParams q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const PwgLayerParams& p = q.f;
    float* bt = smem;
    float* at = smem + 2 * kPwgRes * kPwgLD;
    float* zt = smem;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * 32, b = blockIdx.y;
    const int K1 = 3 * kPwgRes + p.naux, nch1 = K1 / 8;
    const float* xb = p.x + (size_t)b * kPwgRes * p.LS;
    GemmPipe<1, 1, kPwgLD, 64, 6, TileB> pipe1(p.w1p + (size_t)w * nch1 * 64, lane, nch1, TileB{bt + 4 * h * kPwgLD + j, 8 * kPwgLD, nch1});
    pipe1.start_a();
    {
        const int col = tid & 31, r0 = tid >> 5;
        float xv[24], cv[kPwgMaxAux / 8];
#pragma unroll
        for (int i = 0; i < 24; ++i) {
            const int r = r0 + 8 * i, tap = r >> 6, ci = r & 63;
            const int t = t0 + col + (tap - 1) * p.dil;
            const bool ok = (t >= 0) && (t < p.L);
            const float v = xb[(size_t)ci * p.LS + (ok ? t : t0)];
            xv[i] = ok ? v : 0.f;
        }
        const float* cb = p.naux ? p.c + (size_t)b * p.naux * p.LS : nullptr;
        const int tc = t0 + col;
#pragma unroll
        for (int i = 0; i < kPwgMaxAux / 8; ++i) {
            const int r = r0 + 8 * i;
            const bool ok = (r < p.naux) && (tc < p.L);
            cv[i] = 0.f;
            if (ok) cv[i] = cb[(size_t)r * p.LS + tc];
        }
#pragma unroll
        for (int i = 0; i < 24; ++i) bt[(r0 + 8 * i) * kPwgLD + col] = xv[i];
#pragma unroll
        for (int i = 0; i < kPwgMaxAux / 8; ++i)
            if (r0 + 8 * i < p.naux) bt[(3 * kPwgRes + r0 + 8 * i) * kPwgLD + col] = cv[i];
    }
    __syncthreads();
    f32x16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
    pipe1.start_b();
    pipe1.run_blocks(acc, nch1);
    GemmPipe<1, 1, kPwgLD, 64, 6, TileB> pipe2(p.w2p + (size_t)w * 8 * 64, lane, 8, TileB{zt + 4 * h * kPwgLD + j, 8 * kPwgLD, 8});
    pipe2.start_a();
    float b1v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) b1v[r] = p.b1 ? p.b1[32 * w + frag_row(r, h)] : 0.f;
    __syncthreads();
    const int t = t0 + j;
    const bool tv = t < p.L;
    {
        float* ao = q.a_out + (size_t)b * kPwgGate * p.LS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * w + frag_row(r, h);
            const float av = acc[0][0][r] + b1v[r];
            at[row * kPwgLD + j] = av;
            ao[(size_t)row * p.LS + t] = tv ? av : 0.f;             // the one addition to k_pwg_layer
        }
    }
    __syncthreads();
    {
        const int col = tid & 31, r0 = tid >> 5;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = r0 + 8 * i;
            const float xa = at[ch * kPwgLD + col], xg = at[(kPwgRes + ch) * kPwgLD + col];
            const float th = 1.f - 2.f / (__expf(2.f * xa) + 1.f);
            zt[ch * kPwgLD + col] = th * (1.f / (1.f + __expf(-xg)));
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
    pipe2.start_b();
    pipe2.run_blocks(acc, 8);
    if (w < 2) {
        float* xo = p.x_out + (size_t)b * kPwgRes * p.LS;
        const float s = sqrtf(0.5f);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 32 * w + frag_row(r, h);
            const float res = bt[(kPwgRes + ch) * kPwgLD + j];
            const float v = ((acc[0][0][r] + (p.b2 ? p.b2[ch] : 0.f)) + res) * s;
            xo[(size_t)ch * p.LS + t] = tv ? v : 0.f;
        }
    } else {
        float* sk = p.skip + (size_t)b * kPwgRes * p.LS;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 32 * (w - 2) + frag_row(r, h);
            const float hv = acc[0][0][r] + (p.b2 ? p.b2[kPwgRes + ch] : 0.f);
            const size_t idx = (size_t)ch * p.LS + t;
            const float prev = p.first ? 0.f : sk[idx];
            sk[idx] = tv ? prev + hv : 0.f;
        }
    }
}

// ---- gate backward --------------------------------------------------------------------------------------------------------------------------
struct PwgtGateBwdParams {
    const float* dxp;       // [B][64][LS] gradient at the block's residual output, or nullptr (the last block)
    const float* ds;        // [B][64][LS] gradient at the skip sum
    const float* a;         // [B][128][LS] saved gate pre-activations
    const float4* w2tp;     // dsv_pack_weight of [64][128][1]: row ci, columns 0..63 = W_skip[co][ci], 64..127 = W_out[co][ci]
    float* da;              // [B][128][LS]
    int L, LS;
};

__global__ __launch_bounds__(kThreads, 4) void k_pwgt_gate_bwd(const PwgtGateBwdParams p) {
    __shared__ __attribute__((aligned(16))) float gt[kPwgGate * kPwgLD];       // rows 0..63 dS, 64..127 s dx'
    __shared__ __attribute__((aligned(16))) float red[kPwgRes * kPwgLD];       // the second K half's sums, then dz
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = w & 1, kh = w >> 1;
    const int t0 = blockIdx.x * 32, b = blockIdx.y;
    const int nkh = p.dxp ? 2 : 1;
    GemmPipe<1, 1, kPwgLD, 64, 6, TileB> pipe(p.w2tp + (size_t)(rb * 16 + kh * 8) * 64, lane, 8,
                                               TileB{gt + (kh * kPwgRes + 4 * h) * kPwgLD + j, 8 * kPwgLD, 8});
    if (kh < nkh) pipe.start_a();
    const int col = tid & 31, r0 = tid >> 5;
    const int tc = t0 + col;
    const bool cv = tc < p.L;
    {
        const float s = sqrtf(0.5f);
        const size_t base = (size_t)b * kPwgRes * p.LS + tc;
        float v0[8], v1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t idx = base + (size_t)(r0 + 8 * i) * p.LS;
            v0[i] = cv ? p.ds[idx] : 0.f;
            v1[i] = (cv && p.dxp) ? p.dxp[idx] * s : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            gt[(r0 + 8 * i) * kPwgLD + col] = v0[i];
            gt[(kPwgRes + r0 + 8 * i) * kPwgLD + col] = v1[i];
        }
    }
    __syncthreads();
    f32x16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
    if (kh < nkh) {
        pipe.start_b();
        pipe.run_blocks(acc, 8);
    }
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(32 * rb + frag_row(r, h)) * kPwgLD + j] = acc[0][0][r];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* d = red + (32 * rb + frag_row(r, h)) * kPwgLD + j;
            *d = (nkh == 2) ? acc[0][0][r] + *d : acc[0][0][r];
        }
    }
    __syncthreads();
    {
        const float* ab = p.a + (size_t)b * kPwgGate * p.LS + tc;
        float* dab = p.da + (size_t)b * kPwgGate * p.LS + tc;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = r0 + 8 * i;
            const float dz = red[ch * kPwgLD + col];
            const float th = pwgt_tanh(ab[(size_t)ch * p.LS]), sg = pwgt_sigmoid(ab[(size_t)(kPwgRes + ch) * p.LS]);
            const float dt = (dz * sg) * (1.f - th * th);
            const float dg = (dz * th) * (sg * (1.f - sg));
            dab[(size_t)ch * p.LS] = cv ? dt : 0.f;
            dab[(size_t)(kPwgRes + ch) * p.LS] = cv ? dg : 0.f;
        }
    }
}

// ---- dilated convolution backward (data) + conditioning gradient ---------------------------------------------------------------------------
struct PwgtConvBwdParams {
    const float* da;        // [B][128][LS]
    const float* dxp;       // [B][64][LS] or nullptr
    const float4* w1tp;     // dsv_pack_weight of [64][384][1]: row ci, column tap * 128 + co = W_conv[co][ci][tap]
    const float4* wauxtp;   // dsv_pack_weight of [ceil32(naux)][128][1]: row r, column co = W_aux[co][r] (rows >= naux zero), or nullptr
    float* dx;              // [B][64][LS]
    float* dc;              // [B][naux][LS] running sum, or nullptr
    int L, LS, dil, naux, first;
};

__global__ __launch_bounds__(kThreads, 3) void k_pwgt_conv_bwd(const PwgtConvBwdParams p) {
    __shared__ __attribute__((aligned(16))) float bt[3 * kPwgGate * kPwgLD];   // row tap * 128 + co = da[co][t - (tap - 1) dil]; 48 KiB
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = w & 1, kh = w >> 1;
    const int t0 = blockIdx.x * 32, b = blockIdx.y;
    constexpr int nchh = 3 * kPwgGate / 16;                                     // 24 chunks per K half
    GemmPipe<1, 1, kPwgLD, 64, 6, TileB> pipe(p.w1tp + (size_t)(rb * 2 * nchh + kh * nchh) * 64, lane, nchh,
                                               TileB{bt + (kh * nchh * 8 + 4 * h) * kPwgLD + j, 8 * kPwgLD, nchh});
    pipe.start_a();
    {
        const int col = tid & 31, r0 = tid >> 5;
        const float* dab = p.da + (size_t)b * kPwgGate * p.LS;
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int t = t0 + col - (tap - 1) * p.dil;
            const bool ok = (t >= 0) && (t < p.L);
            float v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float x = dab[(size_t)(r0 + 8 * i) * p.LS + (ok ? t : t0)];
                v[i] = ok ? x : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) bt[(tap * kPwgGate + r0 + 8 * i) * kPwgLD + col] = v[i];
        }
    }
    __syncthreads();
    f32x16 acc[1][1], accc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][0][r] = 0.f; accc[0][0][r] = 0.f; }
    pipe.start_b();
    pipe.run_blocks(acc, nchh);
    const int nrbaux = p.dc ? (p.naux + 31) / 32 : 0;
    if (w < nrbaux) {
        // dC rows 32 w .. 32 w + 31 from the centre tile (rows 128..255)
        GemmPipe<1, 1, kPwgLD, 64, 6, TileB> pipec(p.wauxtp + (size_t)w * 16 * 64, lane, 16, TileB{bt + (kPwgGate + 4 * h) * kPwgLD + j, 8 * kPwgLD, 16});
        pipec.start();
        pipec.run_blocks(accc, 16);
    }
    __syncthreads();                                                // every wave is done reading the tile: rows 0..63 take the second K half
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) bt[(32 * rb + frag_row(r, h)) * kPwgLD + j] = acc[0][0][r];
    }
    __syncthreads();
    const int t = t0 + j;
    const bool tv = t < p.L;
    if (kh == 0) {
        const float s = sqrtf(0.5f);
        const size_t base = (size_t)b * kPwgRes * p.LS + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 32 * rb + frag_row(r, h);
            const size_t idx = base + (size_t)ch * p.LS;
            float v = acc[0][0][r] + bt[ch * kPwgLD + j];
            if (p.dxp) v = v + p.dxp[idx] * s;
            p.dx[idx] = tv ? v : 0.f;
        }
    }
    if (w < nrbaux) {
        float* dcb = p.dc + (size_t)b * p.naux * p.LS + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * w + frag_row(r, h);
            if (row < p.naux) {
                float* d = dcb + (size_t)row * p.LS;
                const float prev = p.first ? 0.f : *d;
                *d = tv ? prev + accc[0][0][r] : 0.f;
            }
        }
    }
}

// ---- weight and bias gradients of the 128-row matrices ---------------------------------------------------------------------------------------
struct PwgtWgradParams {
    const float* p0;        // rows 0..63 of P: [B][..][LS] with batch stride bs0 floats, or nullptr (zeros)
    const float* p1;        // rows 64..127 of P, batch stride bs1, or nullptr (zeros: those waves multiply nothing)
    size_t bs0, bs1;
    float scale0;           // rows 0..63 are multiplied by this (s for dx', 1 otherwise)
    const float* x;         // qmode 0: block input [B][64][LS]; qmode 2: the saved activation [B][64][LS]
    const float* c;         // qmode 0: conditioning [B][naux][LS] or nullptr
    const float* a;         // qmode 1: gate pre-activations [B][128][LS]
    float* part;            // [B * nch][128 * N + 128]
    int L, LS, dil, naux, N, nch, qmode;
};

__global__ __launch_bounds__(kThreads, 2) void k_pwgt_wgrad(const PwgtWgradParams p) {
    __shared__ float pt[kPwgGate * kSplitLdw];
    __shared__ float qt[kPwgRes * kSplitLdw];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, g = blockIdx.y;
    const int b = split / p.nch, s0 = (split - b * p.nch) * kSplitK;
    const int s1 = min(p.L, s0 + kSplitK);
    const int col = tid & 31, r0 = tid >> 5;
    const bool live = (w < 2) ? (p.p0 != nullptr) : (p.p1 != nullptr);       // wave-uniform: a missing half of P multiplies nothing
    f32x16 acc[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    float bsum[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) bsum[i] = 0.f;
    const float* p0b = p.p0 ? p.p0 + (size_t)b * p.bs0 : nullptr;
    const float* p1b = p.p1 ? p.p1 + (size_t)b * p.bs1 : nullptr;
    for (int t0 = s0; t0 < s1; t0 += 32) {
        const int t = t0 + col;                                       // < LS: t0 is a multiple of 32 below L
        const bool ok = t < s1;
        float pv[16], qv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = r0 + 8 * i;
            pv[i] = (ok && p0b) ? p0b[(size_t)r * p.LS + t] * p.scale0 : 0.f;
            pv[8 + i] = (ok && p1b) ? p1b[(size_t)r * p.LS + t] : 0.f;
        }
        if (p.qmode == 0) {
            if (g < 3) {
                const int tq = t + (g - 1) * p.dil;
                const bool okq = ok && tq >= 0 && tq < p.L;
                const float* xb = p.x + (size_t)b * kPwgRes * p.LS;
#pragma unroll
                for (int i = 0; i < 8; ++i) qv[i] = okq ? xb[(size_t)(r0 + 8 * i) * p.LS + tq] : 0.f;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = (g - 3) * 64 + r0 + 8 * i;
                    qv[i] = (ok && row < p.naux) ? p.c[((size_t)b * p.naux + row) * p.LS + t] : 0.f;
                }
            }
        } else if (p.qmode == 1) {
            const float* ab = p.a + (size_t)b * kPwgGate * p.LS + t;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ch = r0 + 8 * i;
                qv[i] = ok ? pwgt_tanh(ab[(size_t)ch * p.LS]) * pwgt_sigmoid(ab[(size_t)(kPwgRes + ch) * p.LS]) : 0.f;
            }
        } else {
            const float* xb = p.x + (size_t)b * kPwgRes * p.LS + t;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = ok ? xb[(size_t)(r0 + 8 * i) * p.LS] : 0.f;
                qv[i] = v > 0.f ? v : 0.f;
            }
        }
        __syncthreads();                                              // the previous chunk's LDS reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            pt[(r0 + 8 * i) * kSplitLdw + col] = pv[i];
            pt[(kPwgRes + r0 + 8 * i) * kSplitLdw + col] = pv[8 + i];
            qt[(r0 + 8 * i) * kSplitLdw + col] = qv[i];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) bsum[i] += pv[i];
        __syncthreads();
        if (live) {
            const float* ap = pt + (32 * w + j) * kSplitLdw + h;       // A[i = row][k = t]: lane half h supplies t = 2 s + h
            const float* bp = qt + j * kSplitLdw + h;                  // B[k = t][j = column]
#pragma unroll 4
            for (int s2 = 0; s2 < 16; ++s2) {
                const float a = ap[2 * s2];
                acc[0] = mfma32(a, bp[2 * s2], acc[0]);
                acc[1] = mfma32(a, bp[32 * kSplitLdw + 2 * s2], acc[1]);
            }
        }
    }
    float* out = p.part + (size_t)split * ((size_t)kPwgGate * p.N + kPwgGate);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int n = 64 * g + 32 * nb + j;
        if (n < p.N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[(size_t)(32 * w + frag_row(r, h)) * p.N + n] = acc[nb][r];
        }
    }
    if (g == 0) {                                                     // the 32 threads of a row sit in one half-wave
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float sb = bsum[i];
            sb += __shfl_xor(sb, 1, 64); sb += __shfl_xor(sb, 2, 64); sb += __shfl_xor(sb, 4, 64); sb += __shfl_xor(sb, 8, 64);
            sb += __shfl_xor(sb, 16, 64);
            if (col == 0) out[(size_t)kPwgGate * p.N + (i < 8 ? r0 + 8 * i : kPwgRes + r0 + 8 * (i - 8))] = sb;
        }
    }
}

// ---- vector-shaped pieces -------------------------------------------------------------------------------------------------------------------
// out[2 c] = sum_b sum_t P[b][c][t] q(Q[b][c][t]), out[2 c + 1] = sum_b sum_t P[b][c][t]; a row of P / Q is shared by every channel when its
// channel stride is 0; q = relu when relu_q.  float64: a thread walks its samples in ascending (b, t), then a fixed tree.
__global__ __launch_bounds__(256) void k_pwgt_rowdot(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ out, int B, int L,
                                                     size_t bs_p, size_t cs_p, size_t bs_q, size_t cs_q, int relu_q) {
    const int tid = threadIdx.x, c = blockIdx.x;
    double s[2] = {0.0, 0.0};
    for (int b = 0; b < B; ++b) {
        const float* pr = P + (size_t)b * bs_p + (size_t)c * cs_p;
        const float* qr = Q + (size_t)b * bs_q + (size_t)c * cs_q;
        for (int t = tid; t < L; t += 256) {
            const double pv = (double)pr[t];
            float qv = qr[t];
            if (relu_q) qv = qv > 0.f ? qv : 0.f;
            s[0] += pv * (double)qv;
            s[1] += pv;
        }
    }
    block_sum(s);
    if (tid == 0) { out[2 * c] = (float)s[0]; out[2 * c + 1] = (float)s[1]; }
}

// data gradient of the 64 -> 1 output convolution through the ReLU in front of it: out[b][c][t] = w[c] g[b][t] where saved[b][c][t] > 0
__global__ __launch_bounds__(256) void k_pwgt_last_dgrad(const float* __restrict__ g, const float* __restrict__ saved, const float* __restrict__ w,
                                                         float* __restrict__ out, int C, int L, int LS) {
    const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (t >= LS) return;
    const size_t idx = ((size_t)b * C + c) * LS + t;
    float v = 0.f;
    if (t < L && saved[idx] > 0.f) v = w[c] * g[(size_t)b * LS + t];
    out[idx] = v;
}

// out = scale * g where saved > 0, else 0 (rows of LS samples)
__global__ __launch_bounds__(256) void k_pwgt_relu_mask(const float* __restrict__ g, const float* __restrict__ saved, float* __restrict__ out,
                                                        float scale, int L, int LS) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const size_t r = blockIdx.y;
    if (t >= LS) return;
    const size_t idx = r * LS + t;
    float v = 0.f;
    if (t < L && saved[idx] > 0.f) v = g[idx] * scale;
    out[idx] = v;
}

// upsampling stage (k_pwg_upsample: out[r][t] = sum_j w[j] in[r][(t + j - scale) / scale] for 0 <= t + j - scale < L_out), data gradient:
// din[r][i] = sum_{u in [i scale, (i + 1) scale)} sum_j w[j] g[r][u - j + scale]   (0 <= u - j + scale < L_out); ascending u, then j
__global__ __launch_bounds__(256) void k_pwgt_up_dgrad(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ din, int L_in,
                                                       int LS_in, int scale, int LS_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t r = blockIdx.y;
    if (i >= LS_in) return;
    const int L_out = L_in * scale;
    float s = 0.f;
    if (i < L_in) {
        const float* row = g + r * LS_out;
        for (int u = i * scale; u < (i + 1) * scale; ++u)
            for (int jj = 0; jj <= 2 * scale; ++jj) {
                const int t = u - jj + scale;
                if (t >= 0 && t < L_out) s = fmaf(w[jj], row[t], s);
            }
    }
    din[r * LS_in + i] = s;
}

// filter gradient, per row: part[r][j] = sum_t g[r][t] in[r][(t + j - scale) / scale] in float64 (a thread walks ascending t, then a fixed tree)
__global__ __launch_bounds__(256) void k_pwgt_up_wgrad(const float* __restrict__ g, const float* __restrict__ in, double* __restrict__ part, int L_in,
                                                       int LS_in, int scale, int LS_out) {
    const int tid = threadIdx.x, jj = blockIdx.x;
    const size_t r = blockIdx.y;
    const int L_out = L_in * scale;
    const float* gr = g + r * LS_out;
    const float* ir = in + r * LS_in;
    double s = 0.0;
    for (int t = tid; t < L_out; t += 256) {
        const int u = t + jj - scale;
        if (u >= 0 && u < L_out) s += (double)gr[t] * (double)ir[u / scale];
    }
    s = block_sum(s);
    if (tid == 0) part[r * (2 * scale + 1) + jj] = s;
}

// dw[j] = sum_r part[r][j], ascending r
__global__ __launch_bounds__(256) void k_pwgt_up_wreduce(const double* __restrict__ part, float* __restrict__ dw, int rows, int ntap) {
    const int jj = threadIdx.x;
    if (jj >= ntap) return;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += part[(size_t)r * ntap + jj];
    dw[jj] = (float)s;
}

// conv_in (aux -> aux, kernel K, no padding: L_out = L_in - K + 1) weight gradient: dw[co][ci][k] = sum_b sum_t g[b][co][t] c[b][ci][t + k];
// one thread per element, float64, ascending (b, t).  This runs at the frame rate.
__global__ __launch_bounds__(256) void k_pwgt_convin_wgrad(const float* __restrict__ g, const float* __restrict__ c, float* __restrict__ dw, int B,
                                                           int C, int K, int L_out, int LS_g, int LS_c) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C * C * K) return;
    const int k = i % K, ci = (i / K) % C, co = i / (K * C);
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* gr = g + ((size_t)b * C + co) * LS_g;
        const float* cr = c + ((size_t)b * C + ci) * LS_c + k;
        for (int t = 0; t < L_out; ++t) s += (double)gr[t] * (double)cr[t];
    }
    dw[i] = (float)s;
}

}  // namespace dsd
