// voc_stft_loss.hpp - the multi-resolution STFT loss of the vocoder trainers (C ABI in include/dsv.h, section "STFT loss"; host side in
// voc_stft_loss_abi.hpp): the transpose of the analysis of voc_stft.hpp (the vector-Jacobian product of dsv_stft) and the spectral
// criterion over two spectra, forward and backward.
//
// What is computed, and where the reference computes it (paths relative to the reference root):
//   modules/parallel_wavegan/losses/stft_loss.py:12-31   m = sqrt(clamp(re^2 + im^2, min=1e-7))
//   :52  sc  = ||ym - xm||_F / ||ym||_F        :73  mag = mean |ln ym - ln xm|       (x the prediction, y the recording)
//   :109-153  the mean of both over the resolutions of configs/tts/pwg.yaml:77-82 - on the host side (diffsinger_amd/stft_loss.py).
//
// ADJOINT STFT.  With D[row][f] = sum_n A[row][n] x_pad[f hop + n] (voc_stft.hpp) the cotangent of the padded signal is
//     frame_grad[f][n] = sum_row A[row][n] G[row][f],      dx_pad[t] = sum_f frame_grad[f][t - f hop]
// The first line is the product MODE 2 of k_stft already runs for the inverse - "signal" = a spectrum, rows = samples - against another basis:
// A transposed, i.e. the ANALYSIS window, no 1 / n_fft and no factor 2 on the interior bins (k_stft_make_adj_basis packs it like the inverse
// basis).  The staging of MODE 2 reads Re of bin 0 and of bin n_fft / 2 only: their imaginary cotangents are ignored, as the forward never
// wrote anything but 0 there.  The SAME instantiation k_stft<2, 2> is launched: no new contraction kernel.
// The second line is a gather (k_stft_adj_fold, patterned on k_istft_ola): every output sample adds the frame values of its own position of
// the padded signal in ascending frame order - no division by a window sum - and padding is folded back by the index arithmetic of
// stft_sample read backwards: zero padding drops what fell on it, reflect padding adds to sample u the sums of the positions that mirrored u
// (left: pad_l - u for 1 <= u <= pad_l; right: pad_l + 2 (L - 1) - u for L - 1 - pad_r <= u <= L - 2), direct first, then left, then right.
// A short row (pads < L is all the forward asks) has samples that are mirrored on both sides: the three terms are independent.
//
// SPECTRAL LOSS.  Forward: one pass over X and Y (float2 loads), per-thread float64 sums of (ym - xm)^2, ym^2, |ln ym - ln xm| over a
// grid-stride walk, a fixed-order tree per workgroup (block_sum of block_sum.hpp), partials to a workspace; a one-workgroup second launch adds the partials in index
// order (float64) and writes out[2] plus the two norms the backward needs.  Backward: element-wise,
//     G = (re, im) * [ -g_sc (ym - xm) / (xm S1 S2) - g_mag sign(ln ym - ln xm) / (n P) ]        where P = re^2 + im^2 > 1e-7, else exactly 0
// g_sc, g_mag read from device memory.  sign is taken from the clamped powers (the logarithm and the root are monotone); where ym == xm the
// first term is 0 (also when S1 = 0: x = y gives G = 0, not 0 / 0).
// No atomics, every sum in a fixed order: two calls are bitwise equal.
#pragma once

#include "voc_stft.hpp"
#include "voc_train_common.hpp"

namespace dsd {

constexpr float kStftLossClamp = 1e-7f;
constexpr int kStftLossThreads = 256;
constexpr int kStftLossMaxBlocks = 1024;
constexpr int kStftLossHead = 4;              // doubles in front of the partials: S1 = ||ym - xm||_F, S2 = ||ym||_F, sum |ln ym - ln xm|, n

// The transposed forward basis in the packing of the inverse one (k_stft_make_basis): float4 index ((rt * (N / 8) + kq) * 64 + lane), element e =
// A[row c = (kq * 4 + e) * 2 + (lane >> 5)][sample n], tile row (lane & 31) = 8 g + 4 hh + q holding sample n = rt * 32 + 16 hh + 4 g + q.
__global__ void __launch_bounds__(256) k_stft_make_adj_basis(float* adj, int N, int win) {
    const long long total = (long long)N * N;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int e = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        const long long blk = idx >> 8;
        const int kq = (int)(blk % (N / 8)), rt = (int)(blk / (N / 8));
        const int tr = lane & 31, c = (kq * 4 + e) * 2 + (lane >> 5);
        const int n = rt * 32 + 16 * ((tr >> 2) & 1) + 4 * (tr >> 3) + (tr & 3);
        const int k = c == 1 ? N / 2 : (c >> 1);
        const int m = (int)(((long long)k * n) % N);
        const double w = stft_window(n, N, win);
        adj[idx] = (float)((c == 1 || !(c & 1)) ? w * cospi(2.0 * m / (double)N) : -w * sinpi(2.0 * m / (double)N));
    }
}

struct StftAdjFoldParams {
    const float* frames;      // [B][nF][N]: frame_grad
    float* out;               // [B][L]
    int nF, N, hop, pad_l, pad_r, reflect, L;
};

// sum over the frames that cover position `pos` of the padded signal, ascending
__device__ __forceinline__ float stft_adj_position(const float* fr, long long pos, const StftAdjFoldParams& p) {
    const long long flo = pos - p.N + 1 <= 0 ? 0 : (pos - p.N + p.hop) / p.hop;      // ceil((pos - N + 1) / hop)
    long long fhi = pos / p.hop;
    if (fhi > p.nF - 1) fhi = p.nF - 1;
    float sum = 0.0f;
    for (long long f = flo; f <= fhi; ++f) sum += fr[(size_t)f * p.N + (int)(pos - f * p.hop)];
    return sum;
}

__global__ void __launch_bounds__(256) k_stft_adj_fold(StftAdjFoldParams p) {
    const int b = blockIdx.y;
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= p.L) return;
    const float* fr = p.frames + (size_t)b * p.nF * p.N;
    float sum = stft_adj_position(fr, u + p.pad_l, p);
    if (p.reflect) {
        if (u >= 1 && u <= p.pad_l) sum += stft_adj_position(fr, p.pad_l - u, p);
        if (u <= (long long)p.L - 2 && u >= (long long)p.L - 1 - p.pad_r) sum += stft_adj_position(fr, p.pad_l + 2LL * (p.L - 1) - u, p);
    }
    p.out[(size_t)b * p.L + u] = sum;
}

__global__ void __launch_bounds__(kStftLossThreads) k_stft_loss_partial(const float2* X, const float2* Y, double* ws, long long n) {
    double s[3] = {0.0, 0.0, 0.0};                                           // (ym - xm)^2, ym^2, |ln ym - ln xm|
    for (long long i = (long long)blockIdx.x * kStftLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kStftLossThreads) {
        const float2 x = X[i], y = Y[i];
        const float px = fmaxf(x.x * x.x + x.y * x.y, kStftLossClamp), py = fmaxf(y.x * y.x + y.y * y.y, kStftLossClamp);
        const float xm = sqrtf(px), ym = sqrtf(py);
        const float d = ym - xm;
        s[0] += (double)d * (double)d;
        s[1] += (double)ym * (double)ym;
        s[2] += (double)fabsf(logf(ym) - logf(xm));
    }
    block_sum<3, kStftLossThreads>(s);
    if (threadIdx.x == 0) {
        double* o = ws + kStftLossHead + 3 * (size_t)blockIdx.x;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
}

__global__ void __launch_bounds__(kStftLossThreads) k_stft_loss_final(double* ws, float* out, int nblocks, long long n) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblocks; i += kStftLossThreads) {
        const double* q = ws + kStftLossHead + 3 * (size_t)i;
        s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
    }
    block_sum<3, kStftLossThreads>(s);
    if (threadIdx.x == 0) {
        const double sd = s[0], sy = s[1], sl = s[2];
        const double s1 = sqrt(sd), s2 = sqrt(sy);
        ws[0] = s1; ws[1] = s2; ws[2] = sl; ws[3] = (double)n;
        out[0] = (float)(s1 / s2);                                           // s2 >= sqrt(n * 1e-7) > 0: the clamp
        out[1] = (float)(sl / (double)n);
    }
}

__global__ void __launch_bounds__(kStftLossThreads) k_stft_loss_backward(const float2* X, const float2* Y, const double* ws, const float* g, float2* G,
                                                                         long long n) {
    const float g_sc = g[0], g_mag = g[1];
    const float s12 = (float)(ws[0] * ws[1]), fn = (float)n;
    for (long long i = (long long)blockIdx.x * kStftLossThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kStftLossThreads) {
        const float2 x = X[i], y = Y[i];
        const float p = x.x * x.x + x.y * x.y;
        float2 o = make_float2(0.0f, 0.0f);
        if (p > kStftLossClamp) {
            const float py = fmaxf(y.x * y.x + y.y * y.y, kStftLossClamp);
            const float xm = sqrtf(p), ym = sqrtf(py);
            const float d = ym - xm;
            const float sgn = py > p ? 1.0f : (py < p ? -1.0f : 0.0f);
            float coef = -(g_mag * sgn) / (fn * p);
            if (d != 0.0f) coef -= g_sc * d / (xm * s12);
            o = make_float2(x.x * coef, x.y * coef);
        }
        G[i] = o;
    }
}

}  // namespace dsd
