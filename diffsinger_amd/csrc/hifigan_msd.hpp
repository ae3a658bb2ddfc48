// hifigan_msd.hpp - gfx950 kernels of the HiFi-GAN scale discriminator's stack (modules/hifigan/hifigan.py:253-286: DiscriminatorS - Conv1d 1 -> 128
// (K 15), five grouped strided Conv1d (K 41, padding 20: 128 -> 128 s 2 g 4, 128 -> 256 s 2 g 16, 256 -> 512 s 4 g 16, 512 -> 1024 s 4 g 16,
// 1024 -> 1024 s 1 g 16), a dense 1024 -> 1024 (K 5) and conv_post 1024 -> 1 (K 3), leaky_relu(0.1) between them) forward AND backward.  C ABI in
// include/dsv.h, section "HiFi-GAN scale discriminator stack"; host side in hifigan_msd_abi.hpp.  The dense layer and conv_post are the period
// discriminator's kernels at period 1 (hifigan_mpd.hpp) and are not restated here.
//
// LAYOUT.  Every activation is the reference's own tensor, dense [B][C][L] float32: a feature map is a view of the buffer a kernel wrote, no padding,
// no tail.  Nothing is read or written outside [B][C][L]: a window sample outside [0, L) is a zero in LDS, never a load.
//
//   k_hgs_first / _first_dx / _first_wgrad      the 1 -> C, K = 15 layer on the vector ALU; parameter gradients as float64 partial sums per split of
//                             the position axis (kHgpEdgeSplit positions, the period discriminator's workspace layout, reduced by its
//                             k_hgp_edge_reduce).
//   k_hgs_pack                a layer's weights [Co][Ci / g][41] -> the A stream of k_hgs_gemm (forward, or the data gradient's per-phase matrices).
//   k_hgs_gemm<MT, E>         forward OR data gradient of a grouped layer on the fp32 MFMA (MT = 32: v_mfma_f32_32x32x2_f32, MT = 16:
//                             v_mfma_f32_16x16x4_f32).  A workgroup owns one group, one batch row and NQ columns (64 or 128 positions): RB row blocks x
//                             4 / RB column blocks of MT x MT, one per wave.  The source window of the tile - (NQ - 1) s + 41 samples of each of the
//                             group's source channels - is staged in LDS ONCE, de-interleaved by stride phase: window sample i lies at
//                             [channel][i mod s][i div s], so tap t of consecutive columns j (sample j s + t) is the contiguous run [t mod s][j + t div s].
//                             K order of an output's fma chain: tap, then channel - independent of the batch and of the tile.
//                               forward:        out = leaky_relu(W x + b)
//                               data gradient:  POLYPHASE - input position n = s m + r receives only the taps k = k0 + s u, k0 = (r + 20) mod s, from
//                                               output position m + (r + 20 - k0) / s - u: per phase a stride-1 correlation with 21 / 20 (s = 2) or
//                                               11 / 10 / 10 / 10 (s = 4) taps; no zero-stuffed tensor, no product with a structural zero.  Grid y carries
//                                               (phase, group).  Epilogue (W^T g + cot) * mask(saved).  The 8 input channels per group of the 128 -> 256
//                                               layer fill half of a 16-row block: its other rows are zero rows of the A stream.
//   k_hgs_wgrad<MT, RB>       dW[co][ci][k] = sum_(b, q) G[b][co][q] a[b][ci][q s + k - 20]: a contraction over positions on the MFMA.  A workgroup
//                             owns one group's co_g rows x 8 input channels x 41 taps = 328 columns (the flattened (ci, k) index, MT columns per
//                             block; the window's row stride is 9 mod 32 so that the flattened index walks consecutive banks) over one split of the
//                             units (b, 32 positions); partials to a workspace and k_split_reduce where there is more than one split.
// No atomics, every sum in a fixed order: two calls are bitwise equal.
#pragma once
#include "hifigan_mpd.hpp"

namespace dsd {

constexpr int kHgsK = 41, kHgsPad = 20;                      // the grouped layers
constexpr int kHgsFirstK = 15, kHgsFirstPad = 7;
constexpr int kHgsMaxPhase = 4;
constexpr int kHgsWgCi = 8;                                  // input channels per workgroup of k_hgs_wgrad
constexpr int kHgsWgCols = kHgsWgCi * kHgsK;                 // 328
constexpr int kHgsWgPos = 32;                                // positions per unit
constexpr int kHgsWgGld = 33;                                // LDS row stride of the G tile

typedef float f32x4v __attribute__((ext_vector_type(4)));

// ---- first layer ------------------------------------------------------------------------------------------------------------------------------------
// out[b][c][t] = leaky_relu(bias[c] + sum_k w[c][k] x[b][t + k - 7]); ascending k
__global__ __launch_bounds__(256) void k_hgs_first(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ out, int C, int T, long long ld, float slope) {
    const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const float* xr = x + (size_t)b * ld;
    float v = bias ? bias[c] : 0.f;
#pragma unroll
    for (int k = 0; k < kHgsFirstK; ++k) {
        const int n = t + k - kHgsFirstPad;
        if (n >= 0 && n < T) v = fmaf(w[kHgsFirstK * c + k], xr[n], v);
    }
    out[((size_t)b * C + c) * T + t] = v > 0.f ? v : v * slope;
}

// dx[b][n] = sum_c sum_k w[c][k] g0[b][c][n + 7 - k]; ascending c, then k
__global__ __launch_bounds__(256) void k_hgs_first_dx(const float* __restrict__ g0, const float* __restrict__ w, float* __restrict__ dx, int C, int T) {
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= T) return;
    float v = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* gr = g0 + ((size_t)b * C + c) * T;
#pragma unroll
        for (int k = 0; k < kHgsFirstK; ++k) {
            const int q = n + kHgsFirstPad - k;
            if (q >= 0 && q < T) v = fmaf(w[kHgsFirstK * c + k], gr[q], v);
        }
    }
    dx[(size_t)b * T + n] = v;
}

// part[split][c][k] = sum_n g0[b][c][t] x[b][t + k - 7] (k < 15), part[split][c][15] = sum_n g0 over the split's positions n = (b, t): float64, a
// thread walks its positions in ascending order, then block_sum's tree.  k_hgp_edge_reduce adds the splits.
__global__ __launch_bounds__(256) void k_hgs_first_wgrad(const float* __restrict__ g0, const float* __restrict__ x, float* __restrict__ part, int C, int T,
                                                         long long ld, long long npos) {
    const int tid = threadIdx.x, c = blockIdx.x, split = blockIdx.y;
    const long long n0 = (long long)split * kHgpEdgeSplit, n1 = min(npos, n0 + kHgpEdgeSplit);
    double s[kHgsFirstK + 1];
#pragma unroll
    for (int k = 0; k <= kHgsFirstK; ++k) s[k] = 0.0;
    for (long long n = n0 + tid; n < n1; n += 256) {
        const int b = (int)(n / T), t = (int)(n - (long long)b * T);
        const double gv = (double)g0[((size_t)b * C + c) * T + t];
        const float* xr = x + (size_t)b * ld;
#pragma unroll
        for (int k = 0; k < kHgsFirstK; ++k) {
            const int m = t + k - kHgsFirstPad;
            if (m >= 0 && m < T) s[k] += gv * (double)xr[m];
        }
        s[kHgsFirstK] += gv;
    }
    block_sum(s);
    if (tid == 0) {
        float* o = part + ((size_t)split * C + c) * (kHgsFirstK + 1);
        for (int k = 0; k <= kHgsFirstK; ++k) o[k] = (float)s[k];
    }
}

// ---- MFMA shapes --------------------------------------------------------------------------------------------------------------------------------------
// Mma<32>: v_mfma_f32_32x32x2_f32 - lane (j = lane & 31, kk = lane >> 5) supplies A[row j][k kk] and B[k kk][col j]; D register r is row frag_row(r, kk).
// Mma<16>: v_mfma_f32_16x16x4_f32 - lane (j = lane & 15, kk = lane >> 4) supplies A[row j][k kk] and B[k kk][col j]; D register r is row 4 kk + r.
template <int MT> struct Mma;
template <> struct Mma<32> {
    typedef f32x16 Acc;
    static constexpr int KS = 2, NR = 16;
    static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int r, int kk) { return frag_row(r, kk); }
};
template <> struct Mma<16> {
    typedef f32x4v Acc;
    static constexpr int KS = 4, NR = 4;
    static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int r, int kk) { return 4 * kk + r; }
};

// ---- weight packing ---------------------------------------------------------------------------------------------------------------------------------
// The A stream of k_hgs_gemm: [phase][group][row block][tap][chunk][lane 64][E] floats, element = M[row = rb MT + (lane mod MT)][channel =
// KS (chunk E + e) + lane div MT][tap] of the phase's matrix M (rows x kc channels x ntaps):
//   forward (one phase):  M[co][ci][t] = W[g co_g + co][ci][t]
//   data gradient, phase r:  M[ci][co][t] = W[g co_g + co][ci][k0 + s (nt - 1 - t)] (taps in ascending WINDOW order); rows >= ci_g are zero.
struct HgsPackParams {
    const float* w;         // [Co][ci_g][41]
    float* out;
    int G, co_g, ci_g, S, bwd, MT, E, RB;
    int nphase;
    int k0[kHgsMaxPhase], nt[kHgsMaxPhase];
    long long off[kHgsMaxPhase + 1];                           // float offset of each phase; [nphase]: the total
};

__global__ __launch_bounds__(256) void k_hgs_pack(const HgsPackParams P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.off[P.nphase]) return;
    int ph = 0;
    while (ph + 1 < P.nphase && i >= P.off[ph + 1]) ++ph;
    long long r = i - P.off[ph];
    const int KS = 64 / P.MT, kc = P.bwd ? P.co_g : P.ci_g, ncc = kc / (KS * P.E), nt = P.nt[ph];
    const int e = (int)(r % P.E); r /= P.E;
    const int lane = (int)(r % 64); r /= 64;
    const int cc = (int)(r % ncc); r /= ncc;
    const int t = (int)(r % nt); r /= nt;
    const int rb = (int)(r % P.RB); r /= P.RB;
    const int g = (int)r;
    const int row = rb * P.MT + lane % P.MT, ch = KS * (cc * P.E + e) + lane / P.MT;
    float v = 0.f;
    if (!P.bwd) {
        v = P.w[((size_t)(g * P.co_g + row) * P.ci_g + ch) * kHgsK + t];
    } else if (row < P.ci_g) {
        v = P.w[((size_t)(g * P.co_g + ch) * P.ci_g + row) * kHgsK + P.k0[ph] + P.S * (nt - 1 - t)];
    }
    P.out[i] = v;
}

// ---- forward and data gradient of a grouped layer -------------------------------------------------------------------------------------------------------
struct HgsPhase {
    const float* wp;        // this phase's A stream
    int ntaps;
    int org;                // window sample 0 is source sample col0 * ss + org
    int ro;                 // column c is destination position So * c + ro
    int ncols;              // columns of this phase
};

struct HgsGemmParams {
    const float* src;       // [B][Csrc][Lsrc]
    const float* bias;      // [Cdst] or nullptr (forward)
    const float* cot;       // [B][Cdst][Ldst] or nullptr (data gradient): added before the mask
    const float* saved;     // [B][Cdst][Ldst] post-activation whose mask multiplies the data gradient, or nullptr
    float* dst;             // [B][Cdst][Ldst]
    HgsPhase ph[kHgsMaxPhase];
    int G, Csrc, Lsrc, kc_g, Cdst, Ldst, rows_g, RB;
    int sh;                 // log2 of the de-interleave stride ss of the window (forward: the layer's stride; data gradient: 0)
    int So, PL, CS;         // LDS: [channel: CS][phase: PL][sample div ss]
    float slope;
    int bwd;
};

template <int MT, int E>
__global__ __launch_bounds__(kThreads) void k_hgs_gemm(const HgsGemmParams P) {
    extern __shared__ float hgs_win[];
    typedef Mma<MT> M;
    typedef float VecE __attribute__((ext_vector_type(E)));
    const int g = blockIdx.y % P.G;
    const HgsPhase& ph = P.ph[blockIdx.y / P.G];
    const int b = blockIdx.z;
    const int ncb = 4 / P.RB, NQ = ncb * MT;
    const int col0 = blockIdx.x * NQ;
    if (col0 >= ph.ncols) return;                              // a phase with fewer columns than the grid's widest
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ss = 1 << P.sh, ntaps = ph.ntaps;
    const int WL = (NQ - 1) * ss + ntaps;
    const long long start = (long long)col0 * ss + ph.org;
    // stage the window: wave w takes channels w, w + 4, ..
    for (int c = w; c < P.kc_g; c += 4) {
        const float* sr = P.src + ((size_t)b * P.Csrc + (size_t)g * P.kc_g + c) * P.Lsrc;
        float* wr = hgs_win + c * P.CS;
        for (int i = lane; i < WL; i += 64) {
            const long long n = start + i;
            wr[(i & (ss - 1)) * P.PL + (i >> P.sh)] = (n >= 0 && n < P.Lsrc) ? sr[n] : 0.f;
        }
    }
    __syncthreads();
    const int rb = w % P.RB, cb = w / P.RB;
    const int j = lane % MT, kk = lane / MT;
    const int ncc = P.kc_g / (M::KS * E);
    typename M::Acc acc;
#pragma unroll
    for (int r = 0; r < M::NR; ++r) acc[r] = 0.f;
    const float* bp = hgs_win + kk * P.CS + cb * MT + j;
    const VecE* ap = reinterpret_cast<const VecE*>(ph.wp) + ((size_t)(g * P.RB + rb) * ntaps * ncc) * 64 + lane;
    const int cstep = M::KS * P.CS;
    for (int t = 0; t < ntaps; ++t) {
        const float* bt = bp + (t & (ss - 1)) * P.PL + (t >> P.sh);
        const VecE* at = ap + (size_t)t * ncc * 64;
        for (int cc = 0; cc < ncc; ++cc) {
            const VecE a = at[(size_t)cc * 64];
#pragma unroll
            for (int e = 0; e < E; ++e) acc = M::mma(a[e], bt[(cc * E + e) * cstep], acc);
        }
    }
    const int c = col0 + cb * MT + j;
    if (c >= ph.ncols) return;
    const int pos = P.So * c + ph.ro;
    if (pos >= P.Ldst) return;
#pragma unroll
    for (int r = 0; r < M::NR; ++r) {
        const int row = rb * MT + M::row(r, kk);
        if (row >= P.rows_g) continue;
        const int ch = g * P.rows_g + row;
        const size_t idx = ((size_t)b * P.Cdst + ch) * P.Ldst + pos;
        float v = acc[r];
        if (P.bwd) {
            if (P.cot) v += P.cot[idx];
            if (P.saved) v = v * (P.saved[idx] > 0.f ? 1.f : P.slope);
        } else {
            v += P.bias ? P.bias[ch] : 0.f;
            v = v > 0.f ? v : v * P.slope;
        }
        P.dst[idx] = v;
    }
}

// ---- weight gradient of a grouped layer -----------------------------------------------------------------------------------------------------------------
struct HgsWgradParams {
    const float* g;         // [B][Co][Lout] gradient with respect to the layer's pre-activation
    const float* x;         // [B][Ci][Lin] the layer's input
    float* out;             // [nsplit][Co][ci_g][41] (nsplit = 1: dW itself)
    int B, Co, Ci, co_g, ci_g, Lout, Lin, S;
    int nst;                // units per batch row: ceil(Lout / 32)
    int units, upc;         // B * nst units, `upc` per split
    int CSW;                // LDS row stride of the input window, 9 mod 32
};

template <int MT, int RB>
__global__ __launch_bounds__(kThreads) void k_hgs_wgrad(const HgsWgradParams P) {
    typedef Mma<MT> M;
    constexpr int NCT = (kHgsWgCols + MT - 1) / MT;            // column blocks: 11 (MT 32) or 21 (MT 16)
    constexpr int NA = (NCT + 3) / 4;                          // per wave
    constexpr int CSW_MAX = 169;                               // (32 - 1) * 4 + 41 = 165 -> 9 mod 32
    __shared__ float gt[RB * MT * kHgsWgGld];
    __shared__ float xw[kHgsWgCi * CSW_MAX];
    const int tid = threadIdx.x, lane = tid & 63, j = lane % MT, kk = lane / MT;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cib = blockIdx.x, grp = blockIdx.y, split = blockIdx.z;
    const int u0 = split * P.upc, u1 = min(P.units, u0 + P.upc);
    const int WL = (kHgsWgPos - 1) * P.S + kHgsK;
    typename M::Acc acc[RB][NA];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int r = 0; r < M::NR; ++r) acc[rb][a][r] = 0.f;
    // this lane's column of column block w + 4 a: flattened (ci, tap); a column past the 328 reads column 0 and is not stored
    int boff[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        int c = (w + 4 * a) * MT + j;
        if (c >= kHgsWgCols) c = 0;
        const int ci = c / kHgsK;
        boff[a] = ci * P.CSW + (c - ci * kHgsK) + kk * P.S;
    }
    for (int u = u0; u < u1; ++u) {
        const int b = u / P.nst, q0 = (u - b * P.nst) * kHgsWgPos;
        __syncthreads();                                        // the previous unit's LDS reads are done
        for (int i = tid; i < RB * MT * kHgsWgPos; i += kThreads) {
            const int co = i >> 5, p = i & 31;
            gt[co * kHgsWgGld + p] = (q0 + p < P.Lout) ? P.g[((size_t)b * P.Co + (size_t)grp * P.co_g + co) * P.Lout + q0 + p] : 0.f;
        }
        const long long start = (long long)q0 * P.S - kHgsPad;
        for (int c = w; c < kHgsWgCi; c += 4) {
            const float* xr = P.x + ((size_t)b * P.Ci + (size_t)grp * P.ci_g + cib * kHgsWgCi + c) * P.Lin;
            for (int i = lane; i < WL; i += 64) {
                const long long n = start + i;
                xw[c * P.CSW + i] = (n >= 0 && n < P.Lin) ? xr[n] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int st = 0; st < kHgsWgPos / M::KS; ++st) {
            float av[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) av[rb] = gt[(rb * MT + j) * kHgsWgGld + M::KS * st + kk];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                if ((w + 4 * a) < NCT) {
                    const float bv = xw[boff[a] + M::KS * st * P.S];
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) acc[rb][a] = M::mma(av[rb], bv, acc[rb][a]);
                }
            }
        }
    }
    float* out = P.out + (size_t)split * P.Co * P.ci_g * kHgsK;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const int c = (w + 4 * a) * MT + j;
        if ((w + 4 * a) >= NCT || c >= kHgsWgCols) continue;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int r = 0; r < M::NR; ++r) {
                const int co = grp * P.co_g + rb * MT + M::row(r, kk);
                out[(size_t)co * P.ci_g * kHgsK + (size_t)cib * kHgsWgCols + c] = acc[rb][a][r];
            }
    }
}

}  // namespace dsd
