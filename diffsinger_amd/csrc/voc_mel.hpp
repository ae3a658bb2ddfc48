// voc_mel.hpp - the mel loss of the HiFi-GAN trainer (C ABI in include/dsv.h, section "Mel loss"; host side in voc_mel_abi.hpp): the middle of
// the chain waveform -> spectrum -> magnitude -> mel -> log as a differentiable operator of its own, forward and vector-Jacobian product.
//
// What is computed, and where the reference computes it (paths relative to the reference root):
//   modules/hifigan/mel_utils.py:72-76   spec = sqrt(re^2 + im^2 + 1e-9);  spec = mel_basis @ spec;  log(clamp(spec, min=1e-5))
//   configs/tts/hifigan.yaml lambda_mel  the L1 distance of two such log-mels, the generator's dominant objective - composed on the host side
//                                        (diffsinger_amd/mel_loss.py) from this head, the STFT and its adjoint (voc_stft.hpp, voc_stft_loss.hpp)
//                                        and the L1 mean of the FastSpeech2 losses (dsf_l1_mean).
//
// S is a spectrum [B][n_bins][T][2] - the memory dsv_stft writes - and W a mel basis [M][n_bins], data of the caller, 1 <= M <= 128.  ALL bins
// are treated alike: bins 0 and n_fft / 2 get no special case, whatever imaginary part the caller stored there counts.
//
// HEAD FORWARD (k_mel_head):    mag[k][f] = sqrt(re^2 + im^2 + mag_eps);   mel[f][m] = sum_k W[m][k] mag[k][f];   out[f][m] = log(max(mel, floor))
// on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) with FRAMES AS COLUMNS: the B operand of k-step s is mag[2 s + h][f0 + j] of lane (j, h) - the
// spectrum is read frame-contiguous (32 lanes x 8 bytes), nothing is transposed; the A operand is W[32 mt + j][2 s + h].  One workgroup (4 waves)
// owns 32 frames of one utterance and one 32-row mel tile (grid.z); the k-steps are split into four contiguous runs, one per wave - n_bins is odd,
// so the LAST k-step is half empty (its second slot is a zero operand on both sides) - and the four partial tiles are summed through LDS in the
// fixed order ((w0 + w1) + w2) + w3.  Every summand is non-negative: a plain fp32 accumulator chain is enough here (unlike the DFT, whose partial
// sums wander far above a small total).  The logarithm - natural or base 10 - is evaluated in float64 and rounded once, as k_stft<1, .> does.
// Writes out [B][T][M] (dsv_logmel's layout) and the linear mel [B][T][M] the backward needs.
//
// HEAD BACKWARD (k_mel_head_bwd), cotangent g [B][T][M]:
//     gm[m][f]   = g / mel [/ ln 10]   where the saved mel >= floor, else exactly 0      (torch.clamp(min=): the gradient passes at equality)
//     dmag[k][f] = sum_m W[m][k] gm[m][f]                                               (the transposed product: rows = bins, contraction over m)
//     G[k][f]    = dmag (re, im) / mag,   mag recomputed from S;   exactly 0 where mag == 0 (possible only with mag_eps = 0), not 0 / 0
// One workgroup stages gm of its 32 frames once in LDS ([frame][m], the tile is one contiguous block of g and of mel); every wave then owns ONE
// 32-bin row tile (grid.z covers the tiles four at a time) and runs ceil(M / 2) k-steps: A = W[2 s + h][32 kt + j] (bin-contiguous loads), B from
// LDS.  No wave shares a sum with another.  n_bins is odd: bin n_fft / 2 sits alone in the last row tile, whose other 31 rows are zero operands
// and are never stored.
//
// CLAMP BACKWARD (k_mel_clamp_bwd): dx_out = dx_in where -1 <= x <= 1, else 0 (a NaN x gives 0, as torch's mask does) - the waveform clamp of
// mel_utils.py:59-62 is index arithmetic of the STFT's staging, its mask is applied behind the adjoint (k_stft_adj_fold is not touched).
//
// No atomics, every sum in a fixed order: two calls are bitwise equal.  Nothing allocates or synchronises.
#pragma once

#include "voc_stft.hpp"

namespace dsd {

constexpr int kMelThreads = 256;
constexpr int kMelNF = 32;                    // frames per workgroup: one MFMA column block
constexpr int kMelRedLd = 33;                 // LDS stride of a frame's 32 partial mels (forward)
constexpr int kMelGmLd = kStftMaxMel + 1;     // LDS stride of a frame's gm row (backward)
constexpr float kMelLn10 = 2.30258509299404568402f;

struct MelHeadParams {
    const float2* S;          // spectrum [B][n_bins][T]
    const float* W;           // mel basis [M][n_bins]
    const float* g;           // backward: cotangent [B][T][M]
    const float* mel_in;      // backward: the forward's linear mel [B][T][M]
    float* out;               // forward: log-mel [B][T][M]
    float* mel;               // forward: linear mel [B][T][M]
    float2* G;                // backward: [B][n_bins][T]
    int T, n_bins, M, log10;
    float mag_eps, floor;
};

__device__ __forceinline__ float mel_mag(float2 s, float eps) { return sqrtf((s.x * s.x + s.y * s.y) + eps); }

__global__ void __launch_bounds__(kMelThreads) k_mel_head(MelHeadParams p) {
    __shared__ float red[4 * kMelNF * kMelRedLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, f0 = blockIdx.x * kMelNF, mt = blockIdx.z;
    const int nb = p.n_bins, T = p.T, M = p.M;
    const int nsteps = (nb + 1) / 2, per = (nsteps + 3) / 4;
    const int s0 = wave * per, s1 = min(s0 + per, nsteps);
    const int m = mt * 32 + j, f = f0 + j;
    const bool mrow = m < M, fcol = f < T;
    const float2* S = p.S + (size_t)b * nb * T + (fcol ? f : 0);
    const float* W = p.W + (size_t)(mrow ? m : 0) * nb;

    f32x16 acc = f32x16(0.0f);
    // four k-steps at a time, their loads unconditional (indices clamped into the arrays, the operand zeroed afterwards): nothing keeps a step's
    // loads behind the previous step's MFMA; a step beyond the wave's run multiplies zeros
    for (int sb = s0; sb < s1; sb += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = sb + u, k = 2 * s + h;                          // k == n_bins only in the second slot of the last step
            const int kc = min(k, nb - 1);
            const float w = W[kc];
            const float2 sv = S[(size_t)kc * T];
            const bool kin = s < s1 && k < nb;
            const float a = (kin && mrow) ? w : 0.0f;
            const float mg = (kin && fcol) ? mel_mag(sv, p.mag_eps) : 0.0f;
            acc = mfma32(a, mg, acc);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wave * kMelNF + j) * kMelRedLd + frag_row(r, h)] = acc[r];
    __syncthreads();
    constexpr int W1 = kMelNF * kMelRedLd;
    for (int idx = tid; idx < kMelNF * 32; idx += kMelThreads) {
        const int ml = idx & 31, fl = idx >> 5, mm = mt * 32 + ml, ff = f0 + fl;
        if (mm < M && ff < T) {
            const int at = fl * kMelRedLd + ml;
            const float v = ((red[at] + red[at + W1]) + red[at + 2 * W1]) + red[at + 3 * W1];
            const double x = (double)fmaxf(v, p.floor);
            const size_t o = ((size_t)b * T + ff) * M + mm;
            p.out[o] = (float)(p.log10 ? log10(x) : log(x));
            p.mel[o] = v;
        }
    }
}

__global__ void __launch_bounds__(kMelThreads) k_mel_head_bwd(MelHeadParams p) {
    __shared__ float gm[kMelNF * kMelGmLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, f0 = blockIdx.x * kMelNF;
    const int nb = p.n_bins, T = p.T, M = p.M;
    const int Mp = (M + 1) & ~1;                                          // an odd M: the last k-step's second slot is a zero
    for (int idx = tid; idx < kMelNF * Mp; idx += kMelThreads) {
        const int fl = idx / Mp, m = idx - fl * Mp, ff = f0 + fl;
        float v = 0.0f;
        if (m < M && ff < T) {
            const size_t at = ((size_t)b * T + ff) * M + m;
            const float ml = p.mel_in[at];
            if (ml >= p.floor) {
                v = p.g[at] / ml;
                if (p.log10) v = v / kMelLn10;
            }
        }
        gm[fl * kMelGmLd + m] = v;
    }
    __syncthreads();

    const int kt = blockIdx.z * 4 + wave, ntiles = (nb + 31) / 32;
    if (kt >= ntiles) return;                                             // behind the only barrier
    const int k = kt * 32 + j;
    const bool krow = k < nb;
    const float* W = p.W + (krow ? k : 0);
    f32x16 acc = f32x16(0.0f);
    const int nsteps = Mp / 2;
    for (int sb = 0; sb < nsteps; sb += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int m = 2 * (sb + u) + h;                               // m >= M: a zero operand (the odd M's last slot, the tail of the four)
            const float w = W[(size_t)min(m, M - 1) * nb];                // unconditional load, index clamped; zeroed below
            const float a = (krow && m < M) ? w : 0.0f;
            const float gv = gm[j * kMelGmLd + min(m, M - 1)];
            acc = mfma32(a, m < M ? gv : 0.0f, acc);
        }
    }
    const int f = f0 + j;
    if (f < T) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = kt * 32 + frag_row(r, h);
            if (kk < nb) {
                const size_t at = ((size_t)b * nb + kk) * T + f;
                const float2 s = p.S[at];
                const float mg = mel_mag(s, p.mag_eps);
                float2 o = make_float2(0.0f, 0.0f);
                if (mg > 0.0f) o = make_float2(acc[r] * s.x / mg, acc[r] * s.y / mg);
                p.G[at] = o;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_mel_clamp_bwd(const float* x, const float* dx_in, float* dx_out, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        dx_out[i] = (v >= -1.0f && v <= 1.0f) ? dx_in[i] : 0.0f;
    }
}

}  // namespace dsd
