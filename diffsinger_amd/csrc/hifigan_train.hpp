// hifigan_train.hpp - gfx950 kernels of HiFi-GAN / NSF-HiFi-GAN GENERATOR TRAINING: the backward of every piece of HifiGanGenerator.forward
// (modules/hifigan/hifigan.py:30-92, :104-169; modules/parallel_wavegan/models/source.py:518-531).  The training forward is the inference path's
// one-launch-per-convolution form (k_voc_conv / k_voc_conv_fold): every convolution's input is a tensor in HBM and the leaky ReLU in front of it
// is applied while staging, so the saved pre-activations are buffers that path writes anyway.  C ABI in include/dsv.h, section "HiFi-GAN
// generator training"; host side in hifigan_train_abi.hpp.  Activations are channel-major [B][C][LS] float32, LS = dsv_padded_samples(L); every
// kernel leaves [L, LS) at zero.
//
//   k_hgt_dgrad       dx = (m (*) sum_o sum_k w[o][i][k] g[t - k dil + pad] + residual + sum_in) / divide, m = x_saved > 0 ? 1 : slope: a stride-1
//                     convolution of g with the flipped, transposed filter (W'[i][o][k'] = w[o][i][K - 1 - k'], padding (K - 1) dil - pad) -
//                     k_voc_conv's staging, chunk order and GemmPipe, its own epilogue.  A new kernel: no k_voc_conv instantiation changes.
//   k_hgt_wgrad       dW [rows][K][Ci] = sum_t P(t) Q(t)^T over one split of kSplitK samples of one batch row, 128 rows and 64 columns per
//                     workgroup (k_pwgt_wgrad's tile and step, constants in voc_train_common.hpp).  P = g (a transposed convolution: its
//                     polyphase rows co * u + phase at the input rate), Q column k * Ci + ci = lrelu(x[ci][t + k dil - pad]), the leaky ReLU
//                     applied while staging.  k_split_reduce (voc_train_common.hpp) adds the splits in index order in float64.
//   k_hgt_up_dgrad    transposed convolution, data gradient: dx[ci][q] = m sum_co sum_j w[ci][co][j] g[co][q u + j - p] / divide (a gather)
//   k_hgt_rowsum_part + _reduce / _tanh_bwd / _noise_wgrad / _noise_dhar / _source_mix / _source_bwd
//                     the bias gradients, the output tanh, the noise convolutions and the source module: plain vector-ALU kernels, float64 sums
//                     in a fixed order (block_sum of block_sum.hpp).
// No atomics; every sum runs in a fixed order: two calls are bitwise equal.
#pragma once
#include "voc_kernels.hpp"
#include "voc_train_common.hpp"

namespace dsd {

// ---- convolution data gradient with the mask epilogue -------------------------------------------------------------------------------------
struct HgtDgradParams {
    const float* g;         // [B][Cg][LS] gradient at the convolution's output
    const float4* wp;       // dsv_pack_weight of W' [rows][Cg][KT]
    const float* xs;        // [B][rows][LS] the convolution's saved input (the mask is taken from it), or nullptr: m = 1
    const float* res;       // [B][rows][LS] or nullptr
    const float* sum_in;    // [B][rows][LS] or nullptr
    float* dx;              // [B][rows][LS]
    int Cg, rows, KT, pad, dil, L, LS;      // pad: of the flipped convolution, (K - 1) dil - forward padding
    float slope, divide;
};

// Workgroup = WR = 4 / WT row blocks of 32 x (WT * NB * 32) samples of one utterance, as k_voc_conv.
template <int NB, int WT, int HALO>
__global__ __launch_bounds__(kThreads, 2) void k_hgt_dgrad(const HgtDgradParams p) {
    constexpr int LD = voc_ld<NB, WT, HALO>(), SPAN = voc_span<NB, WT>(), SLAB = voc_slab<NB, WT, HALO>(), WR = 4 / WT;
    constexpr int NCOL4 = LD / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [SLAB][LD]
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w % WR, wt = w / WR;
    const int t0 = blockIdx.x * SPAN, b = blockIdx.y;
    const int rb = blockIdx.z * WR + wr;
    const int nrb = (p.rows + 31) / 32;
    const int rbc = (rb < nrb) ? rb : nrb - 1;                       // waves past the last block walk valid memory and store nothing
    const int ci8 = (p.Cg + 7) / 8;
    const int nchunk_total = ci8 * p.KT;
    f32x16 acc[1][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][nb][r] = 0.f;
    const float* gb = p.g + (size_t)b * p.Cg * p.LS;
    for (int c0 = 0; c0 < p.Cg; c0 += SLAB) {
        const int nc = min(SLAB, p.Cg - c0);
        const int nc8 = (nc + 7) / 8 * 8;                            // rows [nc, nc8) are staged as zeros (their weights are zero too)
        const int nstage = nc8 * NCOL4;
        const int nch = (nc8 / 8) * p.KT;
        const float4* ap = p.wp + ((size_t)rbc * nchunk_total + (size_t)(c0 / 8) * p.KT) * 64;
        VocTapB<LD> bof(smem + 4 * h * LD + HALO + wt * (32 * NB) + j - p.pad, p.KT, p.dil, nch);
        GemmPipe<1, NB, LD, 64, 6, VocTapB<LD>, 1, false, true> pipe(ap, lane, nch, bof);
        pipe.start_a();
        // stage channels [c0, c0 + nc) x samples [t0 - halo, t0 + SPAN + halo), zero outside [0, LS)
        for (int i0 = 0; i0 < nstage; i0 += kVocStageBatch * kThreads) {
            float4 sv[kVocStageBatch];
#pragma unroll
            for (int i = 0; i < kVocStageBatch; ++i) {
                const int idx = i0 + i * kThreads + tid;
                const int row = idx / NCOL4, gq = idx - row * NCOL4;
                const int t = t0 - HALO + 4 * gq;
                const bool ok = idx < nstage && row < nc && t >= 0 && t < p.LS;
                const float4 v = *reinterpret_cast<const float4*>(gb + (size_t)(c0 + (ok ? row : 0)) * p.LS + (ok ? t : 0));
                sv[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            DSD_SB();
#pragma unroll
            for (int i = 0; i < kVocStageBatch; ++i) {
                const int idx = i0 + i * kThreads + tid;
                const int row = idx / NCOL4, gq = idx - row * NCOL4;
                if (idx < nstage) *reinterpret_cast<float4*>(smem + row * LD + 4 * gq) = sv[i];
            }
            DSD_SB();
        }
        __syncthreads();
        pipe.start_b();
        pipe.run_blocks(acc, nch);
        __syncthreads();
    }
    if (rb >= nrb) return;
    const int q0 = t0 + wt * (32 * NB) + j;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = q0 + 32 * nb;
        float xv[16], rv[16], sv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {                               // all the reads first
            const int row = rb * 32 + frag_row(r, h);
            const bool ok = row < p.rows && n < p.LS;
            const size_t o = ((size_t)b * p.rows + (ok ? row : 0)) * p.LS + (ok ? n : 0);
            xv[r] = (p.xs && ok) ? p.xs[o] : 1.f;
            rv[r] = (p.res && ok) ? p.res[o] : 0.f;
            sv[r] = (p.sum_in && ok) ? p.sum_in[o] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rb * 32 + frag_row(r, h);
            const bool ok = row < p.rows && n < p.LS;
            float v = acc[0][nb][r];
            if (p.xs) v = (xv[r] > 0.f) ? v : v * p.slope;
            if (p.res) v = v + rv[r];
            if (p.sum_in) v = v + sv[r];
            if (p.divide != 1.f) v = v / p.divide;
            if (ok) p.dx[((size_t)b * p.rows + row) * p.LS + n] = (n < p.L) ? v : 0.f;
        }
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------------
struct HgtWgradParams {
    const float* g;         // [B][Co][LSg], LSg = LS(L * U)
    const float* x;         // [B][Ci][LSx] the convolution's saved input
    float* part;            // [B * nch][rows][N]
    int Co, U, rows;        // rows = Co * U: row = co * U + phase reads g[co][q U + phase]
    int Ci, K, pad, dil, N; // N = K * Ci columns, column = k * Ci + ci
    int L, LSx, LSg, nch;   // L: samples at the input rate
    float slope;
};

__global__ __launch_bounds__(kThreads, 2) void k_hgt_wgrad(const HgtWgradParams p) {
    __shared__ float pt[128 * kSplitLdw];
    __shared__ float qt[64 * kSplitLdw];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, gc = blockIdx.y, row0 = blockIdx.z * 128;
    const int b = split / p.nch, s0 = (split - b * p.nch) * kSplitK;
    const int s1 = min(p.L, s0 + kSplitK);
    const int col = tid & 31, r0 = tid >> 5;
    const bool live = row0 + 32 * w < p.rows;                         // wave-uniform: rows past the matrix multiply nothing
    f32x16 acc[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    // this thread's 16 rows of P and 8 columns of Q: their channel / phase / tap do not change along the sample axis
    size_t poff[16];
    bool pok[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int R = row0 + r0 + 8 * i;
        pok[i] = R < p.rows;
        const int co = pok[i] ? R / p.U : 0, ph = pok[i] ? R - co * p.U : 0;
        poff[i] = ((size_t)b * p.Co + co) * p.LSg + ph;
    }
    size_t qoff[8];
    int qsh[8];
    bool qok[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = 64 * gc + r0 + 8 * i;
        qok[i] = c < p.N;
        const int k = qok[i] ? c / p.Ci : 0, ci = qok[i] ? c - k * p.Ci : 0;
        qoff[i] = ((size_t)b * p.Ci + ci) * p.LSx;
        qsh[i] = k * p.dil - p.pad;
    }
    for (int t0 = s0; t0 < s1; t0 += 32) {
        const int t = t0 + col;
        const bool ok = t < s1;
        float pv[16], qv[8];
#pragma unroll
        for (int i = 0; i < 16; ++i) pv[i] = (ok && pok[i]) ? p.g[poff[i] + (size_t)t * p.U] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int tq = t + qsh[i];
            const bool okq = ok && qok[i] && tq >= 0 && tq < p.L;
            const float v = okq ? p.x[qoff[i] + tq] : 0.f;
            qv[i] = voc_lrelu(v, p.slope);
        }
        __syncthreads();                                              // the previous chunk's LDS reads are done
#pragma unroll
        for (int i = 0; i < 16; ++i) pt[(r0 + 8 * i) * kSplitLdw + col] = pv[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) qt[(r0 + 8 * i) * kSplitLdw + col] = qv[i];
        __syncthreads();
        if (live) {
            const float* ap = pt + (32 * w + j) * kSplitLdw + h;        // A[i = row][k = t]: lane half h supplies t = 2 s + h
            const float* bp = qt + j * kSplitLdw + h;                   // B[k = t][j = column]
#pragma unroll 4
            for (int s2 = 0; s2 < 16; ++s2) {
                const float a = ap[2 * s2];
                acc[0] = mfma32(a, bp[2 * s2], acc[0]);
                acc[1] = mfma32(a, bp[32 * kSplitLdw + 2 * s2], acc[1]);
            }
        }
    }
    float* out = p.part + (size_t)split * ((size_t)p.rows * p.N);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int n = 64 * gc + 32 * nb + j;
        if (n < p.N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int R = row0 + 32 * w + frag_row(r, h);
                if (R < p.rows) out[(size_t)R * p.N + n] = acc[nb][r];
            }
        }
    }
}

// ---- vector-shaped pieces -------------------------------------------------------------------------------------------------------------------
// out[c] = sum_b sum_t g[b][c][t] in float64, split over the sample axis (one workgroup per channel walked 131 072 samples of the 1-channel
// output layer alone): k_hgt_rowsum_part sums one chunk of kHgtSumChunk samples of one (batch row, channel) - a thread walks ascending t, then a
// fixed tree - into part[c][b][chunk]; k_hgt_rowsum_reduce adds a channel's partials, thread i those at i, i + 256, ..., then the same tree.
constexpr int kHgtSumChunk = 1024;

__global__ __launch_bounds__(256) void k_hgt_rowsum_part(const float* __restrict__ g, double* __restrict__ part, int C, int L, int LS, int nch) {
    const int tid = threadIdx.x, chunk = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int t0 = chunk * kHgtSumChunk, t1 = min(L, t0 + kHgtSumChunk);
    const float* gr = g + ((size_t)b * C + c) * LS;
    double s = 0.0;
    for (int t = t0 + tid; t < t1; t += 256) s += (double)gr[t];
    s = block_sum(s);
    if (tid == 0) part[((size_t)c * gridDim.z + b) * nch + chunk] = s;
}

__global__ __launch_bounds__(256) void k_hgt_rowsum_reduce(const double* __restrict__ part, float* __restrict__ out, int n) {
    const int tid = threadIdx.x, c = blockIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += part[(size_t)c * n + i];
    s = block_sum(s);
    if (tid == 0) out[c] = (float)s;
}

// transposed convolution (stride u, kernel k, padding p) behind a leaky ReLU, data gradient: a stride-u gather of g, ascending (co, j)
__global__ __launch_bounds__(256) void k_hgt_up_dgrad(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ xs,
                                                      float* __restrict__ dx, int Ci, int Co, int u, int k, int pd, int L_in, int LS_in, int L_out,
                                                      int LS_out, float slope, float divide) {
    const int q = blockIdx.x * 256 + threadIdx.x, ci = blockIdx.y, b = blockIdx.z;
    if (q >= LS_in) return;
    const size_t o = ((size_t)b * Ci + ci) * LS_in + q;
    float s = 0.f;
    if (q < L_in) {
        const float* wr = w + (size_t)ci * Co * k;
        for (int co = 0; co < Co; ++co) {
            const float* gr = g + ((size_t)b * Co + co) * LS_out;
            for (int jj = 0; jj < k; ++jj) {
                const int n = q * u + jj - pd;
                if (n >= 0 && n < L_out) s = fmaf(wr[co * k + jj], gr[n], s);
            }
        }
        if (!(xs[o] > 0.f)) s = s * slope;
        if (divide != 1.f) s = s / divide;
    }
    dx[o] = s;
}

// out[b][t] = gy[b][t] (1 - y[b][t]^2): the gradient in front of the output tanh (gy [B][L] unpadded, y / out [B][LS])
__global__ __launch_bounds__(256) void k_hgt_tanh_bwd(const float* __restrict__ gy, const float* __restrict__ y, float* __restrict__ out, int L, int LS) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= LS) return;
    float v = 0.f;
    if (t < L) {
        const float yv = y[(size_t)b * LS + t];
        v = gy[(size_t)b * L + t] * (1.f - yv * yv);
    }
    out[(size_t)b * LS + t] = v;
}

// noise_convs (k_voc_noise_conv: xs[b][c][n] = bias[c] + sum_j w[c][j] har[b][n s - pad + j]) weight gradient, one workgroup per (j, c):
// dw[c][j] = sum_b sum_n g[b][c][n] har[b][n s - pad + j] in float64 (a thread walks ascending (b, n), then a fixed tree)
__global__ __launch_bounds__(256) void k_hgt_noise_wgrad(const float* __restrict__ g, const float* __restrict__ har, float* __restrict__ dw, int B, int C,
                                                         int K, int s, int pad, int Lh, int LSh, int Lo, int LSo) {
    const int tid = threadIdx.x, jj = blockIdx.x, c = blockIdx.y;
    double sum = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* gr = g + ((size_t)b * C + c) * LSo;
        const float* hb = har + (size_t)b * LSh;
        for (int n = tid; n < Lo; n += 256) {
            const long i = (long)n * s - pad + jj;
            if (i >= 0 && i < Lh) sum += (double)gr[n] * (double)hb[i];
        }
    }
    sum = block_sum(sum);
    if (tid == 0) dw[(size_t)c * K + jj] = (float)sum;
}

// its data gradient, accumulated over the stages: dhar[b][i] (+)= sum_c sum_n w[c][i + pad - n s] g[b][c][n], ascending (c, n)
__global__ __launch_bounds__(256) void k_hgt_noise_dhar(const float* __restrict__ g, const float* __restrict__ w, float* __restrict__ dhar, int C, int K,
                                                        int s, int pad, int Lh, int LSh, int Lo, int LSo, int first) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= LSh) return;
    float v = 0.f;
    if (i < Lh) {
        // taps 0 <= i + pad - n s < K  <=>  (i + pad - K) / s < n <= (i + pad) / s
        const int num = i + pad - K + 1;
        int n_lo = num > 0 ? (num + s - 1) / s : 0;
        int n_hi = (i + pad) / s;
        if (n_hi > Lo - 1) n_hi = Lo - 1;
        for (int c = 0; c < C; ++c) {
            const float* gr = g + ((size_t)b * C + c) * LSo;
            const float* wc = w + (size_t)c * K;
            for (int n = n_lo; n <= n_hi; ++n) v = fmaf(wc[i + pad - n * s], gr[n], v);
        }
        if (!first) v = dhar[(size_t)b * LSh + i] + v;
    }
    dhar[(size_t)b * LSh + i] = v;
}

// the uv / noise mix of k_voc_source, written out: sines[b][i][h] = sw[b][h][i] uv + namp noise[b][i][h] (what l_linear multiplies)
struct HgtMixParams {
    const float* f0;        // [B][T]
    const float* sw;        // [B][H][L] dsv_sine_source's workspace: the UNMIXED sines
    const float* noise;     // [B][L][H]
    float* sines;           // [B][L][H]
    int T, up, L, H;
    float noise_std, sine_amp, voiced_threshold;
};

__global__ __launch_bounds__(256) void k_hgt_source_mix(const HgtMixParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= p.L) return;
    const float f = p.f0[(size_t)b * p.T + i / p.up];
    const float uv = (f > p.voiced_threshold) ? 1.f : 0.f;
    const float namp = uv * p.noise_std + ((1.f - uv) * p.sine_amp) / 3.f;          // k_voc_source's expression, operation for operation
    for (int hh = 0; hh < p.H; ++hh) {
        const size_t o = ((size_t)b * p.L + i) * p.H + hh;
        p.sines[o] = p.sw[((size_t)b * p.H + hh) * p.L + i] * uv + namp * p.noise[o];
    }
}

// har = tanh(l_linear(sines)): workgroup h < H: dw[h] = sum_b sum_i dp sines[b][i][h]; workgroup H: db = sum dp; dp = dhar (1 - har^2).
// float64: a thread walks ascending (b, i), then a fixed tree.
__global__ __launch_bounds__(256) void k_hgt_source_bwd(const float* __restrict__ dhar, const float* __restrict__ har, const float* __restrict__ sines,
                                                        float* __restrict__ dw, float* __restrict__ db, int B, int L, int LS, int H) {
    const int tid = threadIdx.x, hh = blockIdx.x;
    double s = 0.0;
    for (int b = 0; b < B; ++b)
        for (int i = tid; i < L; i += 256) {
            const double hv = (double)har[(size_t)b * LS + i];
            const double dp = (double)dhar[(size_t)b * LS + i] * (1.0 - hv * hv);
            s += (hh < H) ? dp * (double)sines[((size_t)b * L + i) * H + hh] : dp;
        }
    s = block_sum(s);
    if (tid == 0) { if (hh < H) dw[hh] = (float)s; else db[0] = (float)s; }
}

}  // namespace dsd
