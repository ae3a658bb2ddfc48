// hifigan_mpd.hpp - gfx950 kernels of the HiFi-GAN period discriminator (modules/hifigan/hifigan.py:181-250: DiscriminatorP - reflect pad to a
// multiple of the period p, view as [B][1][H0][p], five Conv2d((5, 1), stride (3, 1) x 4 then 1, padding (2, 0)) + leaky_relu(0.1), conv_post (3, 1);
// channels 1 -> 32 -> 128 -> 512 -> 1024 -> 1024 -> 1) forward AND backward, and the feature-matching L1 (hifigan.py:328-334).  C ABI in include/dsv.h,
// section "HiFi-GAN period discriminator"; host side in hifigan_mpd_abi.hpp.
//
// LAYOUT.  Every activation is the reference's own tensor, dense [B][C][H][p] float32: a feature map is a view of the buffer a kernel wrote, no
// padding, no tail.  The convolutions run along H only, so position (h, w) of a plane reads (S h + k - 2, w): in the flat plane index q = h p + w
// a tap is the constant offset (k - 2) p.  The GEMM kernels tile the flat position axis n = (b, h, w) of the WHOLE batch: a 64-position tile is full
// whatever H is (H = 10 at p = 11 fills it as H = 51 at p = 2 does); only the last tile of a launch is partial.
//
//   k_hgp_fold / _fold_bwd    reflect pad [B][T] -> [B][H0 p] (the view as [H0][p] is free in this layout) and its adjoint: a reflected sample adds
//                             into its source, dx[t] = g[t] + g[2 (T - 1) - t], source first.
//   k_hgp_first / _first_dx / k_hgp_post / _post_dgrad / k_hgp_edge_wgrad / _edge_reduce      the 1 -> 32 and 1024 -> 1 layers: vector-ALU kernels.
//   k_hgp_gemm                a dense Ci -> Co layer, forward or data gradient, on v_mfma_f32_32x32x2_f32: a 128-row x 64-position tile per workgroup,
//                             wave w owns rows 32 w .. 32 w + 31 and both 32-position blocks.  The A operand is dsv_pack_weight's stream, read
//                             straight into registers (a wave's rows are not shared); the B operand is gathered 32 channels x 64 positions x ONE
//                             tap at a time into LDS (double-buffered, the next block's loads in flight under the MFMAs).
//                               forward:        out = leaky_relu(W x + b), one phase, tap k at h-offset k - 2 of S h
//                               data gradient:  POLYPHASE - grid z = input phase r = h_in mod S, whose positions (m, w), h_in = S m + r, receive only
//                                               the taps k with (r + 2 - k) mod S = 0, from output row m + (r + 2 - k) / S: 1, 2 and 2 taps for
//                                               S = 3 (5 for S = 1), no zero-stuffed tensor and no multiplication by a structural zero.  In the flat
//                                               index of the phase, m p + w, those taps are constant offsets again.  Epilogue: + the cotangent that
//                                               arrives on the feature map, then the mask of the SAVED post-activation (1 where > 0, else slope).
//   k_hgp_wgrad               dW[co][ci][k] = sum_n g[co][n] x[ci][src(n, k)]: a contraction over positions.  A workgroup owns 128 co x 32 ci x 5 taps
//                             (wave w: 32 co, five accumulators) over one split of the position axis; partials to a workspace and k_split_reduce
//                             where there is more than one split (hgp_wgrad_splits, hifigan_mpd_abi.hpp), else straight to dW.
//   k_hgp_bias_grad           db[co] = sum_n g[co][n], float64, block_sum.
//   k_hgp_l1_partial / _final / _bwd      2 sum_pairs mean|r - g|: float64 partial sums in a fixed order; the backward writes +-2 sign(r - g) / numel * g_out.
// No atomics, every sum in a fixed order: two calls are bitwise equal, and a forward value does not depend on the batch it is computed in (the k order
// of an output's fma chain is channel block, tap, channel - independent of the tile the position falls in).
#pragma once
#include "voc_kernels.hpp"
#include "voc_train_common.hpp"

namespace dsd {

constexpr int kHgpK = 5;                                     // taps of the five convs (conv_post: kHgpPostK)
constexpr int kHgpPad = 2;
constexpr int kHgpPostK = 3;
constexpr int kHgpTileM = 128;                               // rows (output channels) per workgroup of k_hgp_gemm
constexpr int kHgpTileN = 64;                                // positions per workgroup
constexpr int kHgpKb = 32;                                   // channels per K block
constexpr int kHgpMaxPhase = 3;                              // the stride
constexpr int kHgpWgM = 128, kHgpWgN = 32, kHgpWgLd = 33;    // k_hgp_wgrad: co x ci per workgroup, LDS row stride
constexpr int kHgpEdgeSplit = 4096;                          // positions per workgroup of k_hgp_edge_wgrad and k_hgs_first_wgrad (hifigan_msd.hpp)
constexpr int kHgpLossThreads = 256, kHgpLossMaxBlocks = 256;

// ---- fold -------------------------------------------------------------------------------------------------------------------------------------
// out[b][i] = x[b][i] (i < T), x[b][2 (T - 1) - i] (T <= i < Tp): F.pad(x, (0, Tp - T), 'reflect'); the host checked Tp - T < T
__global__ __launch_bounds__(256) void k_hgp_fold(const float* __restrict__ x, float* __restrict__ out, int T, long long ld, int Tp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Tp) return;
    const float* r = x + (size_t)blockIdx.y * ld;
    out[(size_t)blockIdx.y * Tp + i] = r[i < T ? i : 2 * (T - 1) - i];
}

// dx[b][t] = g[b][t] + g[b][2 (T - 1) - t] where that index lies in [T, Tp)
__global__ __launch_bounds__(256) void k_hgp_fold_bwd(const float* __restrict__ g, float* __restrict__ dx, int T, int Tp) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const float* r = g + (size_t)blockIdx.y * Tp;
    const int m = 2 * (T - 1) - t;
    float v = r[t];
    if (m >= T && m < Tp) v += r[m];
    dx[(size_t)blockIdx.y * T + t] = v;
}

// ---- first layer (1 -> C, K = 5) and conv_post (C -> 1, K = 3): vector ALU ---------------------------------------------------------------------
// out[b][c][h][w] = leaky_relu(bias[c] + sum_k w[c][k] x[b][S h + k - 2][w]); ascending k
__global__ __launch_bounds__(256) void k_hgp_first(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ out, int C, int Hin, int Hout, int p, int S, float slope) {
    const int q = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (q >= Hout * p) return;
    const int h = q / p, wq = q - h * p;
    const float* xr = x + (size_t)b * Hin * p + wq;
    float v = bias ? bias[c] : 0.f;
#pragma unroll
    for (int k = 0; k < kHgpK; ++k) {
        const int hs = S * h + k - kHgpPad;
        if (hs >= 0 && hs < Hin) v = fmaf(w[kHgpK * c + k], xr[(size_t)hs * p], v);
    }
    out[((size_t)b * C + c) * Hout * p + q] = v > 0.f ? v : v * slope;
}

// dx[b][hi][w] = sum_c sum_k w[c][k] g0[b][c][(hi + 2 - k) / S][w] over the k with S | hi + 2 - k; ascending c, then k
__global__ __launch_bounds__(256) void k_hgp_first_dx(const float* __restrict__ g0, const float* __restrict__ w, float* __restrict__ dx, int C, int Hin,
                                                      int Hout, int p, int S) {
    const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (q >= Hin * p) return;
    const int hi = q / p, wq = q - hi * p;
    int ho[kHgpK];
#pragma unroll
    for (int k = 0; k < kHgpK; ++k) {
        const int d = hi + kHgpPad - k, m = d / S;
        ho[k] = (d >= 0 && m * S == d && m < Hout) ? m : -1;
    }
    float v = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* gr = g0 + ((size_t)b * C + c) * Hout * p + wq;
#pragma unroll
        for (int k = 0; k < kHgpK; ++k)
            if (ho[k] >= 0) v = fmaf(w[kHgpK * c + k], gr[(size_t)ho[k] * p], v);
    }
    dx[(size_t)b * Hin * p + q] = v;
}

// out[b][h][w] = bias[0] + sum_c sum_k w[c][k] a[b][c][h + k - 1][w]; ascending c, then k
__global__ __launch_bounds__(256) void k_hgp_post(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ out, int C, int H, int p) {
    const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (q >= H * p) return;
    const int h = q / p;
    const bool lo = h > 0, hi = h + 1 < H;
    const float* ar = a + (size_t)b * C * H * p + q;
    float v = bias ? bias[0] : 0.f;
    for (int c = 0; c < C; ++c) {
        const float* r = ar + (size_t)c * H * p;
        if (lo) v = fmaf(w[3 * c], r[-p], v);
        v = fmaf(w[3 * c + 1], r[0], v);
        if (hi) v = fmaf(w[3 * c + 2], r[p], v);
    }
    out[(size_t)b * H * p + q] = v;
}

// ga[b][c][h][w] = (sum_k w[c][k] gp[b][h - (k - 1)][w] + cot[b][c][h][w]) m(a[b][c][h][w]);  gp = gp1 (+ gp2): the cotangents of the flattened
// output and of the last feature map, which are the same values
__global__ __launch_bounds__(256) void k_hgp_post_dgrad(const float* __restrict__ gp1, const float* __restrict__ gp2, const float* __restrict__ a,
                                                        const float* __restrict__ w, const float* __restrict__ cot, float* __restrict__ ga, int C, int H,
                                                        int p, float slope) {
    const int q = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (q >= H * p) return;
    const int h = q / p;
    const size_t gi = (size_t)b * H * p + q, idx = ((size_t)b * C + c) * H * p + q;
    auto gp = [&](size_t i) { return gp2 ? gp1[i] + gp2[i] : gp1[i]; };
    float v = w[3 * c + 1] * gp(gi);
    if (h + 1 < H) v = fmaf(w[3 * c], gp(gi + p), v);
    if (h > 0) v = fmaf(w[3 * c + 2], gp(gi - p), v);
    if (cot) v += cot[idx];
    ga[idx] = v * (a[idx] > 0.f ? 1.f : slope);
}

// parameter gradients of both edge layers: part[split][c][k] = sum_n P[n] Q[src(n, k)] (k < KT), part[split][c][KT] = sum_n P[n] over the split's
// positions n = (b, h, w) of P's [Hp][p] planes; Q's planes are [Hq][p], src = (S h + k - pad, w).  First layer: P = g0[b][c] (cs_p = plane),
// Q = x[b] (cs_q = 0); conv_post: P = gp[b] (cs_p = 0; P2 the second cotangent or nullptr), Q = a[b][c].  float64: a thread walks its positions in
// ascending order, then block_sum's tree.
__global__ __launch_bounds__(256) void k_hgp_edge_wgrad(const float* __restrict__ P, const float* __restrict__ P2, const float* __restrict__ Q,
                                                        float* __restrict__ part, int C, int KT, int pad, int S, int Hp, int Hq, int p, long long npos,
                                                        size_t bs_p, size_t cs_p, size_t bs_q, size_t cs_q) {
    const int tid = threadIdx.x, c = blockIdx.x, split = blockIdx.y;
    const long long n0 = (long long)split * kHgpEdgeSplit, n1 = min(npos, n0 + kHgpEdgeSplit);
    const int cpb = Hp * p;
    double s[kHgpK + 1];
#pragma unroll
    for (int k = 0; k <= kHgpK; ++k) s[k] = 0.0;
    for (long long n = n0 + tid; n < n1; n += 256) {
        const int b = (int)(n / cpb), rem = (int)(n - (long long)b * cpb), h = rem / p, wq = rem - h * p;
        const size_t pi = (size_t)b * bs_p + (size_t)c * cs_p + rem;
        const double pv = P2 ? (double)(P[pi] + P2[pi]) : (double)P[pi];
        const float* qr = Q + (size_t)b * bs_q + (size_t)c * cs_q + wq;
#pragma unroll
        for (int k = 0; k < kHgpK; ++k) {
            const int hs = S * h + k - pad;
            if (k < KT && hs >= 0 && hs < Hq) s[k] += pv * (double)qr[(size_t)hs * p];
        }
        s[kHgpK] += pv;
    }
    block_sum(s);
    if (tid == 0) {
        float* o = part + ((size_t)split * C + c) * (KT + 1);
        for (int k = 0; k < KT; ++k) o[k] = (float)s[k];
        o[KT] = (float)s[kHgpK];
    }
}

// dw [C][KT]; db [C] (per_channel_bias) or db [1] = channel 0's sum (conv_post: every channel's workgroups summed the same gp); db may be nullptr
__global__ __launch_bounds__(256) void k_hgp_edge_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int nsplit, int C,
                                                         int KT, int per_channel_bias) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C * (KT + 1)) return;
    const int c = i / (KT + 1), k = i - c * (KT + 1);
    double s = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) s += (double)part[(size_t)sp * C * (KT + 1) + i];
    if (k < KT) dw[c * KT + k] = (float)s;
    else if (db && (per_channel_bias || c == 0)) db[per_channel_bias ? c : 0] = (float)s;
}

// ---- dense layers on MFMA -------------------------------------------------------------------------------------------------------------------------
struct HgpPhase {
    const float4* wp;       // dsv_pack_weight of [rows][Csrc][KT]
    int KT;                 // taps of this phase
    int e[kHgpK];           // tap t reads source row S * hc + e[t]
    int cols_h;             // column rows hc of this phase: columns are (b, hc, w), B * cols_h * p of them
    int ro;                 // column (b, hc, w) is destination row So * hc + ro
};

struct HgpGemmParams {
    const float* src;       // [B][Csrc][Hsrc][p]
    const float* bias;      // [Cdst] or nullptr (forward)
    const float* cot;       // [B][Cdst][Hdst][p] or nullptr (data gradient): added before the mask
    const float* saved;     // [B][Cdst][Hdst][p] post-activation whose mask multiplies the data gradient, or nullptr
    float* dst;             // [B][Cdst][Hdst][p]
    HgpPhase ph[kHgpMaxPhase];
    int B, Csrc, Hsrc, Cdst, Hdst, p, S, So;
    float slope;
    int bwd;
};

__device__ __forceinline__ float f4_at(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

__global__ __launch_bounds__(kThreads, 2) void k_hgp_gemm(const HgpGemmParams P) {
    __shared__ float bt[2][kHgpKb * kHgpTileN];
    const HgpPhase& ph = P.ph[blockIdx.z];
    const int cpb = ph.cols_h * P.p;
    const long long ncols = (long long)P.B * cpb;
    const long long n0 = (long long)blockIdx.x * kHgpTileN;
    if (n0 >= ncols) return;                                   // a phase with fewer columns than the grid's widest
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.y * kHgpTileM + 32 * w;
    const bool rows_ok = row0 < P.Cdst;
    const int KT = ph.KT, nchunk = (P.Csrc / 8) * KT;
    const float4* wrow = ph.wp + ((size_t)(row0 >> 5) * nchunk) * 64 + lane;
    const size_t plane = (size_t)P.Hsrc * P.p;
    // this thread stages column sc, channels sch + 4 i of every K block
    const int sc = tid & 63, sch = tid >> 6;
    const bool cv = n0 + sc < ncols;
    const long long ns = cv ? n0 + sc : 0;
    const int sb = (int)(ns / cpb), srem = (int)(ns - (long long)sb * cpb), shc = srem / P.p, sw = srem - shc * P.p;
    const float* sbase = P.src + (size_t)sb * P.Csrc * plane + sw;
    const int hs0 = P.S * shc;
    const int nkb = (P.Csrc / kHgpKb) * KT;                    // K block kb = (channel block cb, tap t), t fastest

    float bv[8];
    float4 av[4];
    auto fetch = [&](int kb) {
        const int cb = kb / KT, t = kb - cb * KT;
        const int hs = hs0 + ph.e[t];
        const bool ok = cv && hs >= 0 && hs < P.Hsrc;
        const float* s = sbase + (size_t)(ok ? hs : 0) * P.p + (size_t)(cb * kHgpKb + sch) * plane;
#pragma unroll
        for (int i = 0; i < 8; ++i) bv[i] = ok ? s[(size_t)(4 * i) * plane] : 0.f;
        if (rows_ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = wrow[(size_t)((4 * cb + i) * KT + t) * 64];
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    fetch(0);
    for (int kb = 0; kb < nkb; ++kb) {
        float* buf = bt[kb & 1];
        float4 ac[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) buf[(sch + 4 * i) * kHgpTileN + sc] = bv[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) ac[i] = av[i];
        __syncthreads();                                        // buffer kb & 1 is complete; every wave is done with block kb - 1 (the other buffer)
        if (kb + 1 < nkb) fetch(kb + 1);
        if (rows_ok) {
#pragma unroll
            for (int c8 = 0; c8 < 4; ++c8) {
                const float* bp = buf + (8 * c8 + 4 * h) * kHgpTileN + j;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float a = f4_at(ac[c8], s);
                    acc[0] = mfma32(a, bp[s * kHgpTileN], acc[0]);
                    acc[1] = mfma32(a, bp[s * kHgpTileN + 32], acc[1]);
                }
            }
        }
    }
    if (!rows_ok) return;
    const size_t dplane = (size_t)P.Hdst * P.p;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const long long n = n0 + 32 * nb + j;
        if (n >= ncols) continue;
        const int b = (int)(n / cpb), rem = (int)(n - (long long)b * cpb), hc = rem / P.p, wq = rem - hc * P.p;
        const int ho = P.So * hc + ph.ro;
        if (ho >= P.Hdst) continue;
        const size_t base = (size_t)b * P.Cdst * dplane + (size_t)ho * P.p + wq;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + frag_row(r, h);
            const size_t idx = base + (size_t)row * dplane;
            float v = acc[nb][r];
            if (P.bwd) {
                if (P.cot) v += P.cot[idx];
                if (P.saved) v = v * (P.saved[idx] > 0.f ? 1.f : P.slope);
            } else {
                v += P.bias ? P.bias[row] : 0.f;
                v = v > 0.f ? v : v * P.slope;
            }
            P.dst[idx] = v;
        }
    }
}

// ---- weight gradient of a dense layer ---------------------------------------------------------------------------------------------------------------
struct HgpWgradParams {
    const float* g;         // [B][Co][Hout][p] gradient with respect to the layer's pre-activation
    const float* x;         // [B][Ci][Hin][p] the layer's input
    float* out;             // [nsplit][Co][Ci][5] (nsplit = 1: dW itself)
    int B, Co, Ci, Hout, Hin, p, S;
    long long npos, chunk;  // B * Hout * p positions, `chunk` (a multiple of 32) per split
};

__global__ __launch_bounds__(kThreads) void k_hgp_wgrad(const HgpWgradParams P) {
    __shared__ float gt[kHgpWgM * kHgpWgLd];
    __shared__ float xt[kHgpK * kHgpWgN * kHgpWgLd];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int co0 = blockIdx.x * kHgpWgM, ci0 = blockIdx.y * kHgpWgN, split = blockIdx.z;
    const long long nbeg = (long long)split * P.chunk, nend = min(P.npos, nbeg + P.chunk);
    const bool rows_ok = co0 + 32 * w < P.Co;
    const int cpb = P.Hout * P.p;
    const size_t gplane = (size_t)cpb, xplane = (size_t)P.Hin * P.p;
    const int pos = tid & 31, r8 = tid >> 5;                    // this thread stages position `pos` of rows r8 + 8 i
    f32x16 acc[kHgpK];
#pragma unroll
    for (int t = 0; t < kHgpK; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float gv[16], xv[kHgpK][4];
    auto fetch = [&](long long nb) {
        const long long n = nb + pos;
        const bool ok = n < nend;
        const long long nn = ok ? n : 0;
        const int b = (int)(nn / cpb), rem = (int)(nn - (long long)b * cpb), ho = rem / P.p, wq = rem - ho * P.p;
        const float* gb = P.g + ((size_t)b * P.Co + co0 + r8) * gplane + rem;
#pragma unroll
        for (int i = 0; i < 16; ++i) gv[i] = (ok && co0 + r8 + 8 * i < P.Co) ? gb[(size_t)(8 * i) * gplane] : 0.f;
        const float* xb = P.x + ((size_t)b * P.Ci + ci0 + r8) * xplane + wq;
#pragma unroll
        for (int t = 0; t < kHgpK; ++t) {
            const int hs = P.S * ho + t - kHgpPad;
            const bool okx = ok && hs >= 0 && hs < P.Hin;
            const float* xr = xb + (size_t)(okx ? hs : 0) * P.p;
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[t][i] = okx ? xr[(size_t)(8 * i) * xplane] : 0.f;
        }
    };
    if (nbeg < nend) fetch(nbeg);
    for (long long nb = nbeg; nb < nend; nb += 32) {
        __syncthreads();                                        // the previous block's LDS reads are done
#pragma unroll
        for (int i = 0; i < 16; ++i) gt[(r8 + 8 * i) * kHgpWgLd + pos] = gv[i];
#pragma unroll
        for (int t = 0; t < kHgpK; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) xt[(t * kHgpWgN + r8 + 8 * i) * kHgpWgLd + pos] = xv[t][i];
        __syncthreads();
        if (nb + 32 < nend) fetch(nb + 32);
        if (rows_ok) {
            const float* ap = gt + (32 * w + j) * kHgpWgLd + h;         // A[i = co][k = position]: lane half h supplies position 2 s + h
            const float* bp = xt + j * kHgpWgLd + h;                    // B[k = position][j = ci], tap 0
#pragma unroll 4
            for (int s2 = 0; s2 < 16; ++s2) {
                const float a = ap[2 * s2];
#pragma unroll
                for (int t = 0; t < kHgpK; ++t) acc[t] = mfma32(a, bp[t * kHgpWgN * kHgpWgLd + 2 * s2], acc[t]);
            }
        }
    }
    if (!rows_ok) return;
    float* out = P.out + (size_t)split * P.Co * P.Ci * kHgpK;
#pragma unroll
    for (int t = 0; t < kHgpK; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + 32 * w + frag_row(r, h), ci = ci0 + j;
            out[((size_t)co * P.Ci + ci) * kHgpK + t] = acc[t][r];
        }
}

// db[c] = sum_b sum_q g[b][c][q]: float64, a thread walks its positions in ascending order, then block_sum's tree
__global__ __launch_bounds__(256) void k_hgp_bias_grad(const float* __restrict__ g, float* __restrict__ db, int B, int C, int cpb) {
    const int c = blockIdx.x;
    const long long npos = (long long)B * cpb;
    double s = 0.0;
    for (long long n = threadIdx.x; n < npos; n += 256) {
        const int b = (int)(n / cpb), rem = (int)(n - (long long)b * cpb);
        s += (double)g[((size_t)b * C + c) * cpb + rem];
    }
    s = block_sum(s);
    if (threadIdx.x == 0) db[c] = (float)s;
}

// ---- feature-matching L1 ----------------------------------------------------------------------------------------------------------------------------
// ws[block] = sum over the block's elements of |r - g| / n
__global__ void __launch_bounds__(kHgpLossThreads) k_hgp_l1_partial(const float* r, const float* g, double* ws, long long n) {
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * kHgpLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kHgpLossThreads)
        s += fabs((double)r[i] - (double)g[i]);
    s = block_sum<kHgpLossThreads>(s);
    if (threadIdx.x == 0) ws[blockIdx.x] = s / (double)n;
}

// out = 2 sum_i ws[i]: every pair's partial means, in index order per thread, then block_sum's tree
__global__ void __launch_bounds__(kHgpLossThreads) k_hgp_l1_final(const double* ws, float* out, int nblocks) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kHgpLossThreads) s += ws[i];
    s = block_sum<kHgpLossThreads>(s);
    if (threadIdx.x == 0) out[0] = (float)(2.0 * s);
}

// dr = 2 sign(r - g) / n * g_out, dg = -dr; sign(0) = 0
__global__ void __launch_bounds__(kHgpLossThreads) k_hgp_l1_bwd(const float* r, const float* g, const float* gout, float* dr, float* dg, long long n) {
    const float sc = (float)(2.0 * (double)gout[0] / (double)n);
    for (long long i = (long long)blockIdx.x * kHgpLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kHgpLossThreads) {
        const float d = r[i] - g[i];
        const float v = d > 0.f ? sc : d < 0.f ? -sc : 0.f;
        dr[i] = v;
        dg[i] = -v;
    }
}

}  // namespace dsd
