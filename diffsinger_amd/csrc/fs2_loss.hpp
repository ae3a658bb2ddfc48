// fs2_loss.hpp - the training objective of FastSpeech2 (C ABI in include/dsf.h, "FastSpeech2 training objective"); included at the end of
// dsd.hip (one translation unit: shares fail(), HIP_TRY).
//
// What is computed, and where the reference computes it (paths relative to the reference root):
//   k_mel_loss_fwd / k_mel_loss_final   FastSpeech2Task.l1_loss and .ssim_loss (tasks/tts/fs2.py:160-178) on mel_out / target [B,T,M]:
//               the masked L1 numerator, the SSIM map of (x + bias, y + bias) - modules/commons/ssim.py:330-351: an 11 x 11 Gaussian window
//               (sigma 1.5, the 1-D weights of :319-327 in fp32) with ZERO padding of 5 on both axes, C1 = 0.01^2, C2 = 0.03^2 - weighted by
//               weights_nonzero_speech(target) (tasks/tts/tts.py:124-128: a frame counts where any bin of the target is nonzero), and the
//               weight count; one workgroup per (utterance, 16-frame tile) writes four partial sums, one workgroup adds them in a fixed order.
//   k_mel_loss_bwd  d/d mel_out of lam_l1 L1 + lam_ssim (1 - SSIM) (and of the weighted mean of S, the ssim() drop-in): the five local
//               statistics are recomputed from x and y with a halo of 10 frames, then
//                   dx = G * a1 + 2 x (G * a11) + y (G * a12),   a1 / a11 / a12 = c dS/d mu1, c dS/d E11, c dS/d E12,
//               c = dL/dS of the pixel; G symmetric and zero padded, so its adjoint is itself.  The L1 part is sign(x - y) (sign(0) = 0).
//   k_dur_loss_rows / k_dur_loss_final  FastSpeech2Task.add_dur_loss (tasks/tts/fs2.py:180-219) and the MIDI tasks' add_dur_loss
//               (usr/diffsinger_task.py:359-389, :443-473): mel2ph_to_dur as integer counts (modules/fastspeech/tts_modules.py:242-248),
//               pdur / wdur / sdur, and (backward) their gradient wrt dur_pred.  Words are contiguous runs of phones under both segmentations,
//               summed in phone order; the word buffer has T_txt entries, so nothing depends on the data's word count (no host sync).
//
// Every reduction has a fixed order (per-thread strided sums, then block_sum's tree, block_sum.hpp; a kernel's independent sums go through
// it in one call): two evaluations are bitwise equal.  No float atomics.
#pragma once
#include "block_sum.hpp"
#include "loss_math.hpp"

namespace dsd {

constexpr int kMlTile = 16;              // output frames per workgroup
constexpr int kMlMaxM = 128;             // bins held in LDS per row
constexpr int kDurMaxTxt = 2048;         // phones per utterance (LDS per workgroup: 52 bytes per phone)

// gaussian(11, 1.5) of modules/commons/ssim.py:319-322 as torch computes it in fp32 (exp in double, rounded; normalised by the fp32 sum)
__constant__ float kSsimG[11] = {
    0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.106560p-2f,
    0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

struct MelLossParams {
    const float* x; const float* y;      // [B][T][M]: element strides sb / st, bins contiguous
    long long xsb, xst, ysb, yst;
    float* partial;                      // [B * ntile][4]
    float* smap;                         // [B][T][M] contiguous, or null
    const float* stats;                  // bwd: the forward's out[4]
    const float* gout;                   // bwd: DEVICE [3], the upstream gradients of out[0..2]
    const float* gmap;                   // bwd: [B][T][M] dL/dS, or null
    float* dx;                           // bwd: [B][T][M] contiguous
    int T, M, ntile, terms, weighted;    // terms: 1 L1, 2 SSIM
    float bias, lam_l1, lam_ssim;
};

// The arithmetic of the mel kernels is float64 on fp32 operands.  sigma = E - mu^2 cancels against (x + bias)^2 ~ 36 wherever target and
// prediction are flat (padding frames): in fp32 that leaves S good to 1e-5 .. 1e-3 there, no better than any fp32 evaluation, and the
// gradient's three terms cancel likewise.  In float64 the kernels agree with a float64 evaluation to the rounding of the fp32 result.
// The window is the reference's: w1.mm(w1.t()) in fp32 (ssim.py:325-329), every weight the fp32 product of two 1-D weights.
// It is summed directly (121 taps a pixel), not as two 1-D passes: the separable form needs the five row-filtered statistics of 26 rows in
// float64 beside x, y and a1 / a11 / a12 in the backward - 133 + 37 + 78 KiB at M = 128, past the 160 KiB of LDS - and the fp32-rounded
// 2-D weights are not an exact outer product.  Cost (tools/bench_fs2_loss.py): the objective's forward + backward went from 0.18 to 0.27 ms.
__device__ __forceinline__ double ml_w(int k, int l) { return (double)__fmul_rn(kSsimG[k], kSsimG[l]); }

constexpr double kSsimC1 = 0.01 * 0.01;
constexpr double kSsimC2 = 0.03 * 0.03;

// The five local statistics of the pixel whose window starts at row r0 of X / Y [rows][M] (raw values; frame of row 0: tf) and is centred
// on bin m: zero padding outside [0, T) x [0, M) applied after the bias, as F.conv2d pads x + bias.
struct MlStats { double mu1, mu2, e11, e22, e12; };
__device__ __forceinline__ MlStats ml_stats(const float* X, const float* Y, int r0, int tf, int m, int M, int T, double bias) {
    MlStats s{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 11; ++k) {
        const int t = tf + r0 + k;
        if (t < 0 || t >= T) continue;
        for (int l = 0; l < 11; ++l) {
            const int mm = m + l - 5;
            if (mm < 0 || mm >= M) continue;
            const double w = ml_w(k, l);
            const double xv = (double)X[(r0 + k) * M + mm] + bias, yv = (double)Y[(r0 + k) * M + mm] + bias;
            s.mu1 += w * xv;
            s.mu2 += w * yv;
            s.e11 += w * (xv * xv);
            s.e22 += w * (yv * yv);
            s.e12 += w * (xv * yv);
        }
    }
    return s;
}

// k_mel_loss_fwd: grid (ntile, B), 256 threads; dynamic LDS: X, Y [26][M] (raw fp32 values), row flags [16].
__global__ __launch_bounds__(256) void k_mel_loss_fwd(MelLossParams p) {
    extern __shared__ __attribute__((aligned(16))) float ml_sm[];
    const int M = p.M, T = p.T, tid = threadIdx.x;
    const int b = blockIdx.y, t0 = blockIdx.x * kMlTile;
    constexpr int R = kMlTile + 10;
    const bool ssim = (p.terms & 2) != 0;
    const double bias = (double)p.bias;
    float* X = ml_sm;
    float* Y = X + R * M;
    int* wrow = (int*)(Y + R * M);
    const float* xb = p.x + (long long)b * p.xsb;
    const float* yb = p.y + (long long)b * p.ysb;
    if (tid < kMlTile) wrow[tid] = p.weighted ? 0 : 1;
    __syncthreads();
    // rows t0 - 5 .. t0 + 20; rows outside [0, T) are never read (ml_stats skips them: the zero padding)
    for (int i = tid; i < R * M; i += 256) {
        const int r = i / M, m = i - r * M, t = t0 - 5 + r;
        float xv = 0.f, yv = 0.f;
        if (t >= 0 && t < T) {
            xv = xb[(long long)t * p.xst + m];
            yv = yb[(long long)t * p.yst + m];
            if (p.weighted && r >= 5 && r < 5 + kMlTile && yv != 0.f) atomicOr(&wrow[r - 5], 1);
        }
        X[i] = xv;
        Y[i] = yv;
    }
    __syncthreads();
    double a_l1 = 0.0, a_1ms = 0.0, a_s = 0.0;
    for (int i = tid; i < kMlTile * M; i += 256) {
        const int r = i / M, m = i - r * M, t = t0 + r;
        if (t >= T) continue;
        const double w = wrow[r] ? 1.0 : 0.0;
        if (p.terms & 1) a_l1 += fabs((double)X[(r + 5) * M + m] - (double)Y[(r + 5) * M + m]) * w;
        if (ssim) {
            const MlStats s = ml_stats(X, Y, r, t0 - 5, m, M, T, bias);
            const double mu1_sq = s.mu1 * s.mu1, mu2_sq = s.mu2 * s.mu2, mu12 = s.mu1 * s.mu2;
            const double s1 = s.e11 - mu1_sq, s2 = s.e22 - mu2_sq, s12 = s.e12 - mu12;
            const double S = ((2.0 * mu12 + kSsimC1) * (2.0 * s12 + kSsimC2)) / ((mu1_sq + mu2_sq + kSsimC1) * (s1 + s2 + kSsimC2));
            if (p.smap) p.smap[((long long)b * T + t) * M + m] = (float)S;
            a_1ms += (1.0 - S) * w;
            a_s += S * w;
        }
    }
    double tot[3] = {a_l1, a_1ms, a_s};
    block_sum(tot);
    if (tid == 0) {
        int rows = 0;
        for (int r = 0; r < kMlTile && t0 + r < T; ++r) rows += wrow[r];
        float* o = p.partial + ((long long)b * p.ntile + blockIdx.x) * 4;
        o[0] = (float)tot[0]; o[1] = (float)tot[1]; o[2] = (float)tot[2]; o[3] = (float)(rows * M);
    }
}

// k_mel_loss_final: one workgroup; out = [lam_l1 * L1, lam_ssim * (1 - SSIM), mean S, weight count], each a quotient by the count
// (the reference's (l * weights).sum() / weights.sum(), then * lambda).
__global__ __launch_bounds__(256) void k_mel_loss_final(const float* __restrict__ partial, int n, float lam_l1, float lam_ssim, float* __restrict__ out) {
    float tot[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int q = 0; q < 4; ++q) tot[q] = __fadd_rn(tot[q], partial[(long long)i * 4 + q]);
    block_sum(tot);
    if (threadIdx.x == 0) {
        const float cnt = tot[3];
        out[0] = __fmul_rn(__fdiv_rn(tot[0], cnt), lam_l1);
        out[1] = __fmul_rn(__fdiv_rn(tot[1], cnt), lam_ssim);
        out[2] = __fdiv_rn(tot[2], cnt);
        out[3] = cnt;
    }
}

// k_mel_loss_bwd: grid (ntile, B), 256 threads; dynamic LDS: X, Y [36][M] (raw fp32 values), A [3][26][M] float64, row flags [26].
__global__ __launch_bounds__(256) void k_mel_loss_bwd(MelLossParams p) {
    extern __shared__ __attribute__((aligned(16))) float ml_sm[];
    const int M = p.M, T = p.T, tid = threadIdx.x;
    const int b = blockIdx.y, t0 = blockIdx.x * kMlTile;
    constexpr int R2 = kMlTile + 20, R1 = kMlTile + 10;
    const bool ssim = (p.terms & 2) != 0;
    const double bias = (double)p.bias;
    float* X = ml_sm;                                     // raw fp32 values, frames t0 - 10 .. t0 + 25
    float* Y = X + R2 * M;
    double* A = (double*)(Y + R2 * M);                    // a1 | a11 | a12, each [R1][M], frames t0 - 5 .. t0 + 20 (2 R2 M floats: 8-byte aligned)
    int* wrow = (int*)(A + 3 * R1 * M);                   // frames t0 - 5 .. t0 + 20
    const float* xb = p.x + (long long)b * p.xsb;
    const float* yb = p.y + (long long)b * p.ysb;
    const double cnt = (double)p.stats[3];
    const double c_l1 = (double)p.lam_l1 * (double)p.gout[0] / cnt;
    const double c_s = ((double)p.gout[2] - (double)p.lam_ssim * (double)p.gout[1]) / cnt;
    if (tid < R1) wrow[tid] = p.weighted ? 0 : 1;
    __syncthreads();
    for (int i = tid; i < R2 * M; i += 256) {
        const int r = i / M, m = i - r * M, t = t0 - 10 + r;
        float xv = 0.f, yv = 0.f;
        if (t >= 0 && t < T) {
            xv = xb[(long long)t * p.xst + m];
            yv = yb[(long long)t * p.yst + m];
            if (p.weighted && r >= 5 && r < 5 + R1 && yv != 0.f) atomicOr(&wrow[r - 5], 1);
        }
        X[i] = xv;
        Y[i] = yv;
    }
    __syncthreads();
    if (ssim) {
        // a1 / a11 / a12 on frames t0 - 5 .. t0 + 20 (zero outside [0, T): no output pixel there)
        for (int i = tid; i < R1 * M; i += 256) {
            const int r = i / M, m = i - r * M, t = t0 - 5 + r;
            double a1 = 0.0, a11 = 0.0, a12 = 0.0;
            if (t >= 0 && t < T) {
                const long long px = ((long long)b * T + t) * M + m;
                double c = wrow[r] ? c_s : 0.0;
                if (p.gmap) c += (double)p.gmap[px];
                const MlStats s = ml_stats(X, Y, r, t0 - 10, m, M, T, bias);     // X rows r .. r + 10: frames t - 5 .. t + 5
                const double mu1 = s.mu1, mu2 = s.mu2;
                const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const double s1 = s.e11 - mu1_sq, s2 = s.e22 - mu2_sq, s12 = s.e12 - mu12;
                const double An = 2.0 * mu12 + kSsimC1, Bn = 2.0 * s12 + kSsimC2;
                const double Cd = mu1_sq + mu2_sq + kSsimC1, D = s1 + s2 + kSsimC2;
                const double inv_cd = 1.0 / Cd, inv_d = 1.0 / D;
                const double inv_den = inv_cd * inv_d;
                const double S = An * Bn * inv_den;
                // dS/dmu1 = 2 mu2 (Bn - An) / (Cd D) - 2 mu1 S (1/Cd - 1/D);  dS/dE11 = -S / D;  dS/dE12 = 2 An / (Cd D)
                const double dmu1 = 2.0 * mu2 * ((Bn - An) * inv_den) - 2.0 * mu1 * (S * (inv_cd - inv_d));
                a1 = c * dmu1;
                a11 = -(c * (S * inv_d));
                a12 = c * (2.0 * An * inv_den);
            }
            A[i] = a1; A[R1 * M + i] = a11; A[2 * R1 * M + i] = a12;
        }
        __syncthreads();
    }
    for (int i = tid; i < kMlTile * M; i += 256) {
        const int r = i / M, m = i - r * M, t = t0 + r;
        if (t >= T) continue;
        const double xr = (double)X[(r + 10) * M + m], yr = (double)Y[(r + 10) * M + m];
        double g = 0.0;
        if (ssim) {
            // G is symmetric and zero padded: its adjoint is itself.  A rows r .. r + 10 are frames t - 5 .. t + 5 (zero outside [0, T))
            double h1 = 0.0, h11 = 0.0, h12 = 0.0;
            for (int k = 0; k < 11; ++k)
                for (int l = 0; l < 11; ++l) {
                    const int mm = m + l - 5;
                    if (mm < 0 || mm >= M) continue;
                    const double w = ml_w(k, l);
                    const int j = (r + k) * M + mm;
                    h1 += w * A[j];
                    h11 += w * A[R1 * M + j];
                    h12 += w * A[2 * R1 * M + j];
                }
            g = h1 + 2.0 * (xr + bias) * h11 + (yr + bias) * h12;
        }
        if ((p.terms & 1) && wrow[r + 5]) {
            g += c_l1 * loss_sign(xr - yr);
        }
        p.dx[((long long)b * T + t) * M + m] = (float)g;
    }
}

// ------------------------------------------------------------------------------------------------------------
// duration terms
// ------------------------------------------------------------------------------------------------------------
struct DurLossParams {
    const float* dur_pred;               // [B][Tt] log domain
    const long long* mel2ph;             // [B][T]
    const long long* tokens;             // [B][Tt]
    const long long* sil_ids;            // segmentation (a): silence-phone ids [n_sil]
    const long long* wdb;                // segmentation (b): word_boundary [B][Tt]
    float* ws;                           // [B][8] row sums, then [8] totals
    float* out;                          // [3]: pdur, wdur, sdur
    const float* gout;                   // bwd: DEVICE [3]
    float* grad;                         // bwd: [B][Tt]
    int B, Tt, T, n_sil;
    float lam_p, lam_w, lam_s;
};
constexpr int kDurRow = 8;               // floats per row in ws: pnum, pcnt, wnum, wcnt, sterm, bad

// k_dur_loss_rows<BWD>: one workgroup per utterance, 256 threads; dynamic LDS of 5 * Tt + 1 words (padded to 8 bytes) and 4 * Tt float64.
template <bool BWD>
__global__ __launch_bounds__(256) void k_dur_loss_rows(DurLossParams p) {
    extern __shared__ __attribute__((aligned(16))) float dl_sm[];
    __shared__ int itot[256];
    __shared__ int bad;
    const int Tt = p.Tt, T = p.T, tid = threadIdx.x, b = blockIdx.x;
    // The arithmetic is float64 on the fp32 dur_pred: wdur and sdur are (log(a + 1) - log(b + 1))^2 of sums that lie a few percent apart,
    // where one ulp of an fp32 logarithm is already 1e-5 of the loss.
    int* cnt = (int*)dl_sm;                  // [Tt + 1] frames per phone (index 0: padding frames)
    int* raw = cnt + Tt + 1;                 // [Tt] silence flag (a) / word_boundary (b)
    int* cs = raw + Tt;                      // [Tt] inclusive prefix sums of raw
    int* word = cs + Tt;                     // [Tt] word slot in [0, Tt), -1: not in any kept word
    float* D = (float*)(word + Tt);          // [Tt] dur_pred
    double* lin = (double*)(dl_sm + (5 * Tt + 2) / 2 * 2);   // [Tt] (exp(d) - 1).clamp(min=0); 8-byte aligned behind the 5 Tt + 1 words
    double* gt = lin + Tt;                   // [Tt] dur_gt
    double* P = gt + Tt;                     // [Tt] word_dur_p by slot
    double* G = P + Tt;                      // [Tt] word_dur_g by slot
    if (tid == 0) bad = 0;
    for (int i = tid; i <= Tt; i += 256) cnt[i] = 0;
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        const long long v = p.mel2ph[(long long)b * T + t];
        if (v < 0 || v > Tt) bad = 1;                                       // the reference's scatter_add raises
        else atomicAdd(&cnt[v], 1);
    }
    // per phone
    double a_p = 0.0, a_np = 0.0;
    for (int i = tid; i < Tt; i += 256) {
        const long long tok = p.tokens[(long long)b * Tt + i];
        int r;
        if (p.wdb) {
            const long long w = p.wdb[(long long)b * Tt + i];
            if (w < 0 || w > Tt) bad = 1;
            r = (int)(w < 0 ? 0 : w > Tt ? Tt : w);
        } else {
            r = 0;
            for (int k = 0; k < p.n_sil; ++k) r |= (tok == p.sil_ids[k]);
        }
        raw[i] = r;
        D[i] = p.dur_pred[(long long)b * Tt + i];
        P[i] = 0.0;
        G[i] = 0.0;
    }
    __syncthreads();
    for (int i = tid; i < Tt; i += 256) {
        const double np = p.tokens[(long long)b * Tt + i] != 0 ? 1.0 : 0.0;
        const double g = (double)cnt[i + 1] * np;
        const double d = (double)D[i];
        // pdur's target alone is rounded to fp32, like the fp32 dur_pred it is compared with: a prediction that equals logf(dur_gt + 1) then
        // costs exactly 0, as it does in the reference's fp32 evaluation.  (tests/test_gpu_fs2_loss_edges.py builds that prediction with
        // torch.log on the device and relies on it agreeing with logf bit for bit.)  pdur is well conditioned: fp32 here costs < 1e-6.
        const double e = d - (double)logf((float)g + 1.f);
        a_p += e * e * np;
        a_np += np;
        const double l = exp(d) - 1.0;
        lin[i] = l < 0.0 ? 0.0 : l;                                         // clamp(min=0): NaN stays NaN
        gt[i] = g;
    }
    // inclusive scan of raw -> cs (chunk per thread, then the 256 chunk totals)
    const int chunk = (Tt + 255) / 256, c0 = tid * chunk, c1 = min(Tt, c0 + chunk);
    int run = 0;
    for (int i = c0; i < c1; ++i) { run += raw[i]; cs[i] = run; }
    itot[tid] = run;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = tid >= o ? itot[tid - o] : 0;
        __syncthreads();
        itot[tid] += v;
        __syncthreads();
    }
    const int off = tid > 0 ? itot[tid - 1] : 0;
    for (int i = c0; i < c1; ++i) cs[i] += off;
    __syncthreads();
    for (int i = tid; i < Tt; i += 256) {
        int s;
        if (p.wdb) {
            s = cs[i] - raw[i];                                             // F.pad(cumsum(wdb), (1, 0))[:, :-1]: every word kept
            if (s >= Tt) { bad = 1; s = Tt - 1; }                         // word_boundary > 1: more words than phones
        } else {
            s = raw[i] ? -1 : cs[i] - 1;                                    // cumsum(is_sil) * (1 - is_sil), word 0 dropped
        }
        word[i] = s;
    }
    __syncthreads();
    // words are contiguous runs of phones: the first phone of a run sums it in phone order
    double a_w = 0.0, a_m = 0.0;
    for (int i = tid; i < Tt; i += 256) {
        const int s = word[i];
        if (s < 0 || (i > 0 && word[i - 1] == s)) continue;
        double sp = 0.0, sg = 0.0;
        for (int j = i; j < Tt && word[j] == s; ++j) { sp += lin[j]; sg += gt[j]; }
        P[s] = sp;
        G[s] = sg;
        const double m = sg > 0.0 ? 1.0 : 0.0;
        const double e = log(sp + 1.0) - log(sg + 1.0);
        a_w += e * e * m;
        a_m += m;
    }
    double a_sp = 0.0, a_sg = 0.0;
    for (int i = tid; i < Tt; i += 256) { a_sp += lin[i]; a_sg += gt[i]; }
    // one block_sum for the kernel: the forward's six sums, of which the backward needs the first two (its array is a third of the size)
    double sums[BWD ? 2 : 6] = {a_sp, a_sg};
    if constexpr (!BWD) { sums[2] = a_p; sums[3] = a_np; sums[4] = a_w; sums[5] = a_m; }
    block_sum(sums);
    const double S = sums[0], Sg = sums[1];
    const double es = log(S + 1.0) - log(Sg + 1.0);
    if constexpr (!BWD) {
        if (tid == 0) {
            float* o = p.ws + (long long)b * kDurRow;
            o[0] = (float)sums[2]; o[1] = (float)sums[3]; o[2] = (float)sums[4]; o[3] = (float)sums[5]; o[4] = (float)(es * es); o[5] = bad ? 1.f : 0.f;
        }
        return;
    }
    // P / G of every slot are written: block_sum's barriers lie behind the loop that fills them
    const float* tot = p.ws + (long long)p.B * kDurRow;                      // pcnt, wcnt, bad (k_dur_loss_final)
    const float nanv = __int_as_float(0x7fc00000);
    const double cp = (double)p.gout[0] * (double)p.lam_p * 2.0 / (double)tot[0];
    const double cw = (double)p.gout[1] * (double)p.lam_w * 2.0 / (double)tot[1];
    const double csd = (double)p.gout[2] * (double)p.lam_s * 2.0 * es / ((S + 1.0) * (double)p.B);
    for (int i = tid; i < Tt; i += 256) {
        const double np = p.tokens[(long long)b * Tt + i] != 0 ? 1.0 : 0.0;
        const double d = (double)D[i], g = gt[i];
        double gd = cp * (d - (double)logf((float)g + 1.f)) * np;
        double gl = csd;
        const int s = word[i];
        if (s >= 0) {
            const double sp = P[s], sg = G[s];
            const double m = sg > 0.0 ? 1.0 : 0.0;
            const double e = log(sp + 1.0) - log(sg + 1.0);
            gl += cw * e * m / (sp + 1.0);
        }
        const double ex = exp(d);
        const double dl = (ex - 1.0 >= 0.0) ? ex : 0.0;                     // clamp_min's backward passes where input >= min
        gd += gl * dl;
        p.grad[(long long)b * Tt + i] = (bad || tot[2] != 0.f) ? nanv : (float)gd;
    }
}

// k_dur_loss_final: one workgroup; sums the rows in utterance order.  Any mel2ph (or word_boundary) value outside its range: NaN losses.
__global__ __launch_bounds__(64) void k_dur_loss_final(DurLossParams p) {
    if (threadIdx.x != 0) return;
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < p.B; ++b)
        for (int q = 0; q < 6; ++q) s[q] = __fadd_rn(s[q], p.ws[(long long)b * kDurRow + q]);
    const float nanv = __int_as_float(0x7fc00000);
    const bool bad = s[5] != 0.f;
    p.out[0] = bad ? nanv : __fmul_rn(__fdiv_rn(s[0], s[1]), p.lam_p);
    p.out[1] = bad ? nanv : __fmul_rn(__fdiv_rn(s[2], s[3]), p.lam_w);
    p.out[2] = bad ? nanv : __fmul_rn(__fdiv_rn(s[4], (float)p.B), p.lam_s);
    float* tot = p.ws + (long long)p.B * kDurRow;
    tot[0] = s[1]; tot[1] = s[3]; tot[2] = s[5];
}

}  // namespace dsd

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
static inline size_t ml_lds_fwd(int M) { return (size_t)2 * (kMlTile + 10) * M * 4 + kMlTile * 4; }
static inline size_t ml_lds_bwd(int M) {
    const int R2 = kMlTile + 20, R1 = kMlTile + 10;
    return (size_t)2 * R2 * M * 4 + (size_t)3 * R1 * M * 8 + R1 * 4;
}
static inline size_t dl_ints(int Tt) { return ((size_t)5 * Tt + 2) / 2 * 2; }      // cnt, raw, cs, word, D: 5 Tt + 1 words, padded to 8 bytes
static inline size_t dl_lds(int Tt) { return dl_ints(Tt) * 4 + (size_t)4 * Tt * 8; }
// dynamic LDS beyond 64 KiB must be allowed per kernel (M = 128: 26 / 114 KiB; T_txt = 2048: 104 KiB); block_sum's static array comes on
// top (k_mel_loss_fwd: 6 KiB; k_dur_loss_rows: 12 KiB forward, 4 KiB backward), the workgroup's 160 KiB bound the sum
static int fl_lds_attr() {
    static bool done = false;
    if (!done) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_mel_loss_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ml_lds_fwd(kMlMaxM)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_mel_loss_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ml_lds_bwd(kMlMaxM)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_dur_loss_rows<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl_lds(kDurMaxTxt)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_dur_loss_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl_lds(kDurMaxTxt)));
        done = true;
    }
    return DSD_OK;
}

extern "C" int64_t dsf_fs2_loss_workspace_floats(int32_t B, int32_t T, int32_t which) {
    if (B < 1 || B > 65535 || T < 1) return -1;
    if (which == 0) return (int64_t)B * ((T + kMlTile - 1) / kMlTile) * 4;
    if (which == 1) return (int64_t)B * kDurRow + 8;
    return -1;
}

static int ml_check(const char* who, const float* x, const float* y, int32_t B, int32_t T, int32_t M, int32_t terms) {
    if (!x || !y || B < 1 || B > 65535 || T < 1 || T > (1 << 26) || M < 1 || M > kMlMaxM || terms < 1 || terms > 3)
        return fail(DSD_ERR_INVALID, "%s: bad argument (B=%d T=%d M=%d terms=%d; 1 <= M <= %d, terms 1 (L1) | 2 (SSIM))", who, B, T, M, terms, kMlMaxM);
    return DSD_OK;
}

extern "C" int dsf_mel_loss(const float* x, int64_t x_sb, int64_t x_st, const float* y, int64_t y_sb, int64_t y_st, int32_t B, int32_t T, int32_t M,
                            float bias, int32_t weighted, int32_t terms, float lam_l1, float lam_ssim, float* ssim_map, float* workspace, float* out,
                            void* stream) {
    DSD_TRY(ml_check("dsf_mel_loss", x, y, B, T, M, terms));
    if (!workspace || !out || (ssim_map && !(terms & 2))) return fail(DSD_ERR_INVALID, "dsf_mel_loss: workspace / out missing, or a map without the SSIM term");
    MelLossParams p{};
    p.x = x; p.y = y; p.xsb = x_sb; p.xst = x_st; p.ysb = y_sb; p.yst = y_st;
    p.partial = workspace; p.smap = ssim_map;
    p.T = T; p.M = M; p.ntile = (T + kMlTile - 1) / kMlTile; p.terms = terms; p.weighted = weighted ? 1 : 0;
    p.bias = bias; p.lam_l1 = lam_l1; p.lam_ssim = lam_ssim;
    DSD_TRY(fl_lds_attr());
    hipLaunchKernelGGL(k_mel_loss_fwd, dim3((unsigned)p.ntile, (unsigned)B), dim3(256), ml_lds_fwd(M), (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mel_loss_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, B * p.ntile, lam_l1, lam_ssim, out);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_mel_loss_bwd(const float* x, int64_t x_sb, int64_t x_st, const float* y, int64_t y_sb, int64_t y_st, int32_t B, int32_t T, int32_t M,
                                float bias, int32_t weighted, int32_t terms, float lam_l1, float lam_ssim, const float* stats, const float* grad_out,
                                const float* grad_map, float* dx, void* stream) {
    DSD_TRY(ml_check("dsf_mel_loss_bwd", x, y, B, T, M, terms));
    if (!stats || !grad_out || !dx || (grad_map && !(terms & 2))) return fail(DSD_ERR_INVALID, "dsf_mel_loss_bwd: stats / grad_out / dx missing, or a map without the SSIM term");
    MelLossParams p{};
    p.x = x; p.y = y; p.xsb = x_sb; p.xst = x_st; p.ysb = y_sb; p.yst = y_st;
    p.stats = stats; p.gout = grad_out; p.gmap = grad_map; p.dx = dx;
    p.T = T; p.M = M; p.ntile = (T + kMlTile - 1) / kMlTile; p.terms = terms; p.weighted = weighted ? 1 : 0;
    p.bias = bias; p.lam_l1 = lam_l1; p.lam_ssim = lam_ssim;
    DSD_TRY(fl_lds_attr());
    hipLaunchKernelGGL(k_mel_loss_bwd, dim3((unsigned)p.ntile, (unsigned)B), dim3(256), ml_lds_bwd(M), (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

static int dl_params(const char* who, DurLossParams& p, const float* dur_pred, const int64_t* mel2ph, const int64_t* txt_tokens, const int64_t* sil_ids,
                     int32_t n_sil, const int64_t* word_boundary, int32_t B, int32_t T_txt, int32_t T, float lam_ph, float lam_word, float lam_sent,
                     float* workspace) {
    if (!dur_pred || !mel2ph || !txt_tokens || !workspace || B < 1 || B > 65535 || T_txt < 1 || T_txt > kDurMaxTxt || T < 1 || n_sil < 0 ||
        (word_boundary && sil_ids) || (!word_boundary && n_sil > 0 && !sil_ids))
        return fail(DSD_ERR_INVALID, "%s: bad argument (B=%d T_txt=%d T=%d n_sil=%d; T_txt <= %d; silence ids or word_boundary, not both)", who, B, T_txt,
                    T, n_sil, kDurMaxTxt);
    p = DurLossParams{};
    p.dur_pred = dur_pred; p.mel2ph = (const long long*)mel2ph; p.tokens = (const long long*)txt_tokens;
    p.sil_ids = (const long long*)sil_ids; p.n_sil = word_boundary ? 0 : n_sil; p.wdb = (const long long*)word_boundary;
    p.ws = workspace; p.B = B; p.Tt = T_txt; p.T = T; p.lam_p = lam_ph; p.lam_w = lam_word; p.lam_s = lam_sent;
    return DSD_OK;
}

extern "C" int dsf_dur_loss(const float* dur_pred, const int64_t* mel2ph, const int64_t* txt_tokens, const int64_t* sil_ids, int32_t n_sil,
                            const int64_t* word_boundary, int32_t B, int32_t T_txt, int32_t T, float lam_ph, float lam_word, float lam_sent,
                            float* workspace, float* out, void* stream) {
    DurLossParams p;
    DSD_TRY(dl_params("dsf_dur_loss", p, dur_pred, mel2ph, txt_tokens, sil_ids, n_sil, word_boundary, B, T_txt, T, lam_ph, lam_word, lam_sent, workspace));
    if (!out) return fail(DSD_ERR_INVALID, "dsf_dur_loss: out missing");
    p.out = out;
    DSD_TRY(fl_lds_attr());
    hipLaunchKernelGGL(k_dur_loss_rows<false>, dim3((unsigned)B), dim3(256), dl_lds(T_txt), (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_dur_loss_final, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_dur_loss_bwd(const float* dur_pred, const int64_t* mel2ph, const int64_t* txt_tokens, const int64_t* sil_ids, int32_t n_sil,
                                const int64_t* word_boundary, int32_t B, int32_t T_txt, int32_t T, float lam_ph, float lam_word, float lam_sent,
                                const float* workspace, const float* grad_out, float* grad, void* stream) {
    DurLossParams p;
    DSD_TRY(dl_params("dsf_dur_loss_bwd", p, dur_pred, mel2ph, txt_tokens, sil_ids, n_sil, word_boundary, B, T_txt, T, lam_ph, lam_word, lam_sent,
                      (float*)workspace));
    if (!grad_out || !grad) return fail(DSD_ERR_INVALID, "dsf_dur_loss_bwd: grad_out / grad missing");
    p.gout = grad_out; p.grad = grad;
    DSD_TRY(fl_lds_attr());
    hipLaunchKernelGGL(k_dur_loss_rows<true>, dim3((unsigned)B), dim3(256), dl_lds(T_txt), (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
