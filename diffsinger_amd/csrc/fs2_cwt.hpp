// fs2_cwt.hpp - the CWT pitch path of FastSpeech2 (pitch_type: cwt; C ABI in include/dsf.h, "CWT pitch"); included at the end of dsd.hip (one
// translation unit: shares fail(), HIP_TRY).
//
// What is computed, and where the reference computes it (paths relative to the reference root):
//   k_cwt2f0        FastSpeech2.cwt2f0_norm (modules/fastspeech/fs2.py:239-245): utils/cwt.py:118-125 inverse_cwt_torch (the weighted sum of
//                   the 10 scales, then (rec - mean) / unbiased std along the frames), :135-147 cwt2f0 (affine in the utterance's mean / std,
//                   exp), the repeat of the last frame up to mel2ph's width, utils/pitch_utils.py:34-42 norm_f0.  One workgroup per row.
//   k_cwt2f0_bwd    its gradient with respect to the scales, mean and std; the row statistics are the forward's (saved), everything else is
//                   recomputed.  One workgroup per row, two block sums (the tail, then both statistics at once), one pass of stores.
//   k_cwt_loss_partial / k_cwt_loss_final / k_cwt_loss_bwd   the cwt branch of FastSpeech2Task.add_pitch_loss (tasks/tts/fs2.py:233-247):
//                   C (l1 / l2 mean over the 10 scale channels), uv (masked BCE with logits on the last channel), f0_mean, f0_std (l1 means).
//
// The arithmetic is float64 on fp32 operands (as the mel kernels of fs2_loss.hpp): these are a few thousand values per row, bound by launch
// latency, and the exp behind the affine map amplifies the rounding of its argument (|y| ~ 7: half an fp32 ulp of y is 2.4e-7 of f0).
//
// The reduction-order rule: a row's statistics are summed by thread i over the frames i, i + 256, ... below N (the frames that enter the
// statistics), then by block_sum's tree over the 256 threads (block_sum.hpp).  N is all that order depends on - not the allocated width
// T, not T_out - so a forward on a frame budget and a forward on the exact axis carry the same bits on the frames they share.  No atomics
// anywhere.
#pragma once
#include "block_sum.hpp"
#include "loss_math.hpp"

namespace dsd {

constexpr int kCwtBlock = 256;           // threads of every kernel here (block_sum's THREADS)
constexpr int kCwtScales = 10;           // scales of the wavelet decomposition (utils/cwt.py: len(cwt_scales))
constexpr int kCwtLossBlocks = 256;      // partial blocks of the loss

struct CwtParams {
    const float* cwt;        // [B][T][10], element strides sb / st / sc
    long long sb, st, sc;
    const float* mean;       // [B]
    const float* std;        // [B]
    const float* live;       // DEVICE scalar (frame_keep's count) or nullptr: the statistics run over the first live[0] frames
    float* out;              // fwd: [B][T_out]
    double* stats;           // [B][2]: mu, 1 / sigma (written by the forward, read by the backward)
    const float* dout;       // bwd: [B][T_out]
    float* dcwt;             // bwd: [B][T][10], element strides gsb / gst / gsc
    long long gsb, gst, gsc;
    float* dmean;            // bwd: [B]
    float* dstd;             // bwd: [B]
    double w[kCwtScales];    // (k + 3.5)^-2.5 rounded to fp32 (the reference's weights)
    int T, T_out, norm;      // norm: 1 standard, 2 log
    float std_scale, f0_mean, f0_std;
};

__device__ __forceinline__ double cwt_rec(const CwtParams& p, const float* row, int t) {
    const float* c = row + (long long)t * p.st;
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < kCwtScales; ++k) r = fma((double)c[k * p.sc], p.w[k], r);
    return r;
}

__device__ __forceinline__ int cwt_live(const CwtParams& p) {
    if (!p.live) return p.T;
    const float l = p.live[0];
    return l >= (float)p.T ? p.T : (l > 0.f ? (int)l : 0);      // NaN counts as 0 frames: the statistics are NaN then, as a 0 / 0 is
}

__global__ __launch_bounds__(kCwtBlock) void k_cwt2f0(const CwtParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = p.cwt + (long long)b * p.sb;
    const int N = cwt_live(p);
    double s = 0.0;
    for (int t = tid; t < N; t += kCwtBlock) s += cwt_rec(p, row, t);
    const double mu = block_sum<kCwtBlock>(s) / (double)N;
    double d = 0.0;
    for (int t = tid; t < N; t += kCwtBlock) { const double e = cwt_rec(p, row, t) - mu; d = fma(e, e, d); }
    const double rs = 1.0 / sqrt(block_sum_again<kCwtBlock>(d) / (double)(N - 1));
    if (tid == 0) { p.stats[2 * b] = mu; p.stats[2 * b + 1] = rs; }
    const double sd = (double)p.std[b] * (double)p.std_scale, mean = (double)p.mean[b];
    float* o = p.out + (long long)b * p.T_out;
    for (int t = tid; t < p.T_out; t += kCwtBlock) {
        const int tt = t < p.T ? t : p.T - 1;                   // torch.cat([f0] + [f0[:, -1:]] * (T_out - T), 1)
        const double z = (cwt_rec(p, row, tt) - mu) * rs;
        const double f0 = exp(fma(z, sd, mean));
        o[t] = (float)(p.norm == 2 ? log2(f0) : (f0 - (double)p.f0_mean) / (double)p.f0_std);
    }
}

// With N the frames of the statistics, L = {t < N}, s = std * std_scale, z_t = (rec_t - mu) / sigma for EVERY t < T:
//   dy_t = d out_t / ln 2 (log)  or  d out_t * f0_t / f0_std (standard), the padded columns' d out added to t = T - 1
//   d mean = sum_t dy_t,  d std = std_scale sum_t dy_t z_t,  dz_t = s dy_t
//   d rec_j = (dz_j - [j in L] (sum_t dz_t / N + z_j sum_t dz_t z_t / (N - 1))) / sigma
// both sums over all T frames: a frame outside L has no share in mu and sigma, but its z depends on them, and that dependence lands on
// the frames of L (d mu / d rec_j = 1 / N, d sigma / d rec_j = z_j / (N - 1) for j in L, 0 otherwise).
__global__ __launch_bounds__(kCwtBlock) void k_cwt2f0_bwd(const CwtParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = p.cwt + (long long)b * p.sb;
    const float* g = p.dout + (long long)b * p.T_out;
    const int N = cwt_live(p);
    const double mu = p.stats[2 * b], rs = p.stats[2 * b + 1];
    const double sd = (double)p.std[b] * (double)p.std_scale, mean = (double)p.mean[b];
    double tail = 0.0;
    for (int t = p.T + tid; t < p.T_out; t += kCwtBlock) tail += (double)g[t];
    tail = block_sum<kCwtBlock>(tail);
    const double c_log = 1.0 / 0.693147180559945309417, c_std = 1.0 / (double)p.f0_std;
    double ab[2] = {0.0, 0.0};              // sum dy, sum dy z
    for (int t = tid; t < p.T; t += kCwtBlock) {
        const double z = (cwt_rec(p, row, t) - mu) * rs;
        const double gt = (double)g[t] + (t == p.T - 1 ? tail : 0.0);
        const double dy = p.norm == 2 ? gt * c_log : gt * exp(fma(z, sd, mean)) * c_std;
        ab[0] += dy;
        ab[1] = fma(dy, z, ab[1]);
    }
    block_sum_again<2, kCwtBlock>(ab);
    const double a = ab[0], bz = ab[1];
    if (tid == 0) { p.dmean[b] = (float)a; p.dstd[b] = (float)((double)p.std_scale * bz); }
    const double ka = a / (double)N, kb = bz / (double)(N - 1);
    float* drow = p.dcwt + (long long)b * p.gsb;
    for (int t = tid; t < p.T; t += kCwtBlock) {
        const double z = (cwt_rec(p, row, t) - mu) * rs;
        const double gt = (double)g[t] + (t == p.T - 1 ? tail : 0.0);
        const double dy = p.norm == 2 ? gt * c_log : gt * exp(fma(z, sd, mean)) * c_std;
        const double drec = sd * (t < N ? dy - (ka + z * kb) : dy) * rs;
        float* dc = drow + (long long)t * p.gst;
#pragma unroll
        for (int k = 0; k < kCwtScales; ++k) dc[k * p.gsc] = (float)(drec * p.w[k]);
    }
}

struct CwtLossParams {
    const float* pred;       // [B][T][Cp] the predictor's output, element strides sb / st / sc; Cp >= 10 (+ 1 with use_uv: the LAST channel)
    long long sb, st, sc;
    const float* spec;       // [B][T][10] contiguous
    const float* uv;         // [B][T] contiguous (use_uv) or nullptr
    const long long* mel2ph; // [B][T] contiguous; nonpadding = mel2ph != 0 (use_uv) or nullptr
    const float* mean_pred; const float* mean_tgt; const float* std_pred; const float* std_tgt;      // [B]
    double* partial;         // [nblk][3]: C numerator, uv numerator, sum nonpadding
    float* out;              // [5]: C, uv, f0_mean, f0_std, sum nonpadding
    const float* gout;       // bwd: DEVICE [4]
    float* dpred;            // bwd: [B][T][Cp] contiguous
    float* dmean;            // bwd: [B]
    float* dstd;             // bwd: [B]
    long long n;             // B * T
    int B, T, Cp, nblk, use_uv, l2;
    float lam_f0, lam_uv;
};

__global__ __launch_bounds__(kCwtBlock) void k_cwt_loss_partial(const CwtLossParams p) {
    double a_c = 0.0, a_uv = 0.0, a_np = 0.0;
    for (long long i = blockIdx.x * (long long)kCwtBlock + threadIdx.x; i < p.n; i += (long long)gridDim.x * kCwtBlock) {
        const long long b = i / p.T, t = i - b * p.T;
        const float* pr = p.pred + b * p.sb + t * p.st;
        const float* sp = p.spec + i * kCwtScales;
#pragma unroll
        for (int k = 0; k < kCwtScales; ++k) {
            const double d = (double)pr[k * p.sc] - (double)sp[k];
            a_c += p.l2 ? d * d : fabs(d);
        }
        if (p.use_uv) {
            const double w = p.mel2ph[i] != 0 ? 1.0 : 0.0;
            const double x = (double)pr[(long long)(p.Cp - 1) * p.sc], z = (double)p.uv[i];
            a_uv += bce_logits(x, z) * w;
            a_np += w;
        }
    }
    double tot[3] = {a_c, a_uv, a_np};
    block_sum<3, kCwtBlock>(tot);
    if (threadIdx.x == 0) {
        double* o = p.partial + (size_t)blockIdx.x * 3;
        o[0] = tot[0]; o[1] = tot[1]; o[2] = tot[2];
    }
}

__global__ __launch_bounds__(kCwtBlock) void k_cwt_loss_final(const CwtLossParams p) {
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};       // the three partial columns, |d mean|, |d std|
    for (int i = threadIdx.x; i < p.nblk; i += kCwtBlock) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] += p.partial[(size_t)i * 3 + k];
    }
    for (int b = threadIdx.x; b < p.B; b += kCwtBlock) {
        a[3] += fabs((double)p.mean_pred[b] - (double)p.mean_tgt[b]);
        a[4] += fabs((double)p.std_pred[b] - (double)p.std_tgt[b]);
    }
    block_sum<5, kCwtBlock>(a);
    const double t0 = a[0], t1 = a[1], t2 = a[2], m = a[3], s = a[4];
    if (threadIdx.x == 0) {
        p.out[0] = (float)(t0 / ((double)p.n * kCwtScales) * (double)p.lam_f0);
        p.out[1] = p.use_uv ? (float)(t1 / t2 * (double)p.lam_uv) : 0.f;         // an empty mask is 0 / 0 = NaN, as the reference's expression
        p.out[2] = (float)(m / (double)p.B * (double)p.lam_f0);
        p.out[3] = (float)(s / (double)p.B * (double)p.lam_f0);
        p.out[4] = (float)t2;
    }
}

// the gradient of the WHOLE parent tensor in one pass (scale channels, the uv logit, zeros between them) and of the two statistics
__global__ __launch_bounds__(kCwtBlock) void k_cwt_loss_bwd(const CwtLossParams p, const float* __restrict__ stats) {
    const double c_c = (double)p.gout[0] * (double)p.lam_f0 / ((double)p.n * kCwtScales);
    const double c_uv = p.use_uv ? (double)p.gout[1] * (double)p.lam_uv / (double)stats[4] : 0.0;
    for (long long i = blockIdx.x * (long long)kCwtBlock + threadIdx.x; i < p.n; i += (long long)gridDim.x * kCwtBlock) {
        const long long b = i / p.T, t = i - b * p.T;
        const float* pr = p.pred + b * p.sb + t * p.st;
        const float* sp = p.spec + i * kCwtScales;
        float* dp = p.dpred + i * p.Cp;
#pragma unroll
        for (int k = 0; k < kCwtScales; ++k) {
            const double d = (double)pr[k * p.sc] - (double)sp[k];
            dp[k] = (float)(c_c * (p.l2 ? 2.0 * d : loss_sign(d)));
        }
        for (int k = kCwtScales; k < p.Cp; ++k) dp[k] = 0.f;
        if (p.use_uv) {
            const double w = p.mel2ph[i] != 0 ? 1.0 : 0.0;
            const double x = (double)pr[(long long)(p.Cp - 1) * p.sc], z = (double)p.uv[i];
            dp[p.Cp - 1] = (float)(c_uv * (w * bce_logits_grad(x, z)));
        }
    }
    if (blockIdx.x == 0) {
        const double c_m = (double)p.gout[2] * (double)p.lam_f0 / (double)p.B, c_s = (double)p.gout[3] * (double)p.lam_f0 / (double)p.B;
        for (int b = threadIdx.x; b < p.B; b += kCwtBlock) {
            p.dmean[b] = (float)(c_m * loss_sign((double)p.mean_pred[b] - (double)p.mean_tgt[b]));
            p.dstd[b] = (float)(c_s * loss_sign((double)p.std_pred[b] - (double)p.std_tgt[b]));
        }
    }
}

}  // namespace dsd

// ------------------------------------------------------------------------------------------------------------
// host side (C ABI in include/dsf.h)
// ------------------------------------------------------------------------------------------------------------
static int cwt_params(dsd::CwtParams& p, const char* what, const float* cwt, int64_t sb, int64_t st, int64_t sc, const float* mean, const float* std,
                      const float* live, double* stats, int32_t B, int32_t T, int32_t T_out, float std_scale, int32_t pitch_norm, float f0_mean,
                      float f0_std) {
    if (!cwt || !mean || !std || !stats) return fail(DSD_ERR_INVALID, "%s: null argument", what);
    if (B < 1 || B > 65535 || T < 1 || T_out < T || (pitch_norm != 1 && pitch_norm != 2))
        return fail(DSD_ERR_INVALID, "%s: bad argument (B=%d T=%d T_out=%d pitch_norm=%d; 1 <= B <= 65535, 1 <= T <= T_out, pitch_norm 1 standard / 2 log)",
                    what, B, T, T_out, pitch_norm);
    if (pitch_norm == 1 && !(f0_std != 0.f)) return fail(DSD_ERR_INVALID, "%s: f0_std must be nonzero under pitch_norm standard", what);
    p.cwt = cwt; p.sb = sb; p.st = st; p.sc = sc; p.mean = mean; p.std = std; p.live = live; p.stats = stats; p.T = T; p.T_out = T_out;
    p.norm = pitch_norm; p.std_scale = std_scale; p.f0_mean = f0_mean; p.f0_std = f0_std;
    // utils/cwt.py:120: (arange.float() + 1 + 2.5) ** -2.5 - the reference's weights are fp32 values (whatever the dtype of the scales they
    // multiply), each the correctly rounded power
    for (int k = 0; k < dsd::kCwtScales; ++k) p.w[k] = (double)(float)std::pow((double)k + 3.5, -2.5);
    return DSD_OK;
}

extern "C" int dsf_cwt2f0(const float* cwt, int64_t sb, int64_t st, int64_t sc, const float* mean, const float* std, const float* live, float* out,
                          double* stats, int32_t B, int32_t T, int32_t T_out, float std_scale, int32_t pitch_norm, float f0_mean, float f0_std,
                          void* stream) {
    using namespace dsd;
    if (!out) return fail(DSD_ERR_INVALID, "dsf_cwt2f0: null argument");
    CwtParams p{};
    const int rc = cwt_params(p, "dsf_cwt2f0", cwt, sb, st, sc, mean, std, live, stats, B, T, T_out, std_scale, pitch_norm, f0_mean, f0_std);
    if (rc != DSD_OK) return rc;
    p.out = out;
    hipLaunchKernelGGL(k_cwt2f0, dim3((unsigned)B), dim3(kCwtBlock), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_cwt2f0_bwd(const float* cwt, int64_t sb, int64_t st, int64_t sc, const float* mean, const float* std, const float* live,
                              const double* stats, const float* d_out, float* d_cwt, int64_t gsb, int64_t gst, int64_t gsc, float* d_mean,
                              float* d_std, int32_t B, int32_t T, int32_t T_out, float std_scale, int32_t pitch_norm, float f0_mean, float f0_std,
                              void* stream) {
    using namespace dsd;
    if (!d_out || !d_cwt || !d_mean || !d_std) return fail(DSD_ERR_INVALID, "dsf_cwt2f0_bwd: null argument");
    CwtParams p{};
    const int rc = cwt_params(p, "dsf_cwt2f0_bwd", cwt, sb, st, sc, mean, std, live, const_cast<double*>(stats), B, T, T_out, std_scale, pitch_norm,
                              f0_mean, f0_std);
    if (rc != DSD_OK) return rc;
    p.dout = d_out; p.dcwt = d_cwt; p.gsb = gsb; p.gst = gst; p.gsc = gsc; p.dmean = d_mean; p.dstd = d_std;
    hipLaunchKernelGGL(k_cwt2f0_bwd, dim3((unsigned)B), dim3(kCwtBlock), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsf_cwt_pitch_loss_workspace_floats(void) { return (int64_t)dsd::kCwtLossBlocks * 3 * 2; }      // doubles, counted in floats

static int cwt_loss_params(dsd::CwtLossParams& p, const char* what, const float* pred, int64_t sb, int64_t st, int64_t sc, const float* cwt_spec,
                           const float* uv, const int64_t* mel2ph, const float* mean_pred, const float* mean_tgt, const float* std_pred,
                           const float* std_tgt, int32_t B, int32_t T, int32_t channels, int32_t use_uv, int32_t l2, float lam_f0, float lam_uv) {
    if (!pred || !cwt_spec || !mean_pred || !mean_tgt || !std_pred || !std_tgt || (use_uv && (!uv || !mel2ph)))
        return fail(DSD_ERR_INVALID, "%s: null argument", what);
    if (B < 1 || T < 1 || channels < dsd::kCwtScales + (use_uv ? 1 : 0))
        return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d T=%d channels=%d use_uv=%d; %d scale channels, the uv logit behind them)", what, B, T,
                    channels, use_uv, dsd::kCwtScales);
    p.pred = pred; p.sb = sb; p.st = st; p.sc = sc; p.spec = cwt_spec; p.uv = use_uv ? uv : nullptr;
    p.mel2ph = use_uv ? reinterpret_cast<const long long*>(mel2ph) : nullptr;
    p.mean_pred = mean_pred; p.mean_tgt = mean_tgt; p.std_pred = std_pred; p.std_tgt = std_tgt;
    p.n = (long long)B * T; p.B = B; p.T = T; p.Cp = channels; p.use_uv = use_uv ? 1 : 0; p.l2 = l2 ? 1 : 0; p.lam_f0 = lam_f0; p.lam_uv = lam_uv;
    p.nblk = (int)std::min<long long>(dsd::kCwtLossBlocks, (p.n + dsd::kCwtBlock - 1) / dsd::kCwtBlock);
    return DSD_OK;
}

extern "C" int dsf_cwt_pitch_loss(const float* pred, int64_t sb, int64_t st, int64_t sc, const float* cwt_spec, const float* uv, const int64_t* mel2ph,
                                  const float* f0_mean_pred, const float* f0_mean, const float* f0_std_pred, const float* f0_std, int32_t B,
                                  int32_t T, int32_t channels, int32_t use_uv, int32_t l2, float lam_f0, float lam_uv, float* workspace, float* out,
                                  void* stream) {
    using namespace dsd;
    if (!workspace || !out) return fail(DSD_ERR_INVALID, "dsf_cwt_pitch_loss: null argument");
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return fail(DSD_ERR_INVALID, "dsf_cwt_pitch_loss: the workspace must be 8-byte aligned");
    CwtLossParams p{};
    const int rc = cwt_loss_params(p, "dsf_cwt_pitch_loss", pred, sb, st, sc, cwt_spec, uv, mel2ph, f0_mean_pred, f0_mean, f0_std_pred, f0_std, B, T,
                                   channels, use_uv, l2, lam_f0, lam_uv);
    if (rc != DSD_OK) return rc;
    p.partial = reinterpret_cast<double*>(workspace); p.out = out;
    hipLaunchKernelGGL(k_cwt_loss_partial, dim3((unsigned)p.nblk), dim3(kCwtBlock), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(k_cwt_loss_final, dim3(1), dim3(kCwtBlock), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_cwt_pitch_loss_bwd(const float* pred, int64_t sb, int64_t st, int64_t sc, const float* cwt_spec, const float* uv,
                                      const int64_t* mel2ph, const float* f0_mean_pred, const float* f0_mean, const float* f0_std_pred,
                                      const float* f0_std, int32_t B, int32_t T, int32_t channels, int32_t use_uv, int32_t l2, float lam_f0,
                                      float lam_uv, const float* stats, const float* grad_out, float* d_pred, float* d_f0_mean_pred,
                                      float* d_f0_std_pred, void* stream) {
    using namespace dsd;
    if (!stats || !grad_out || !d_pred || !d_f0_mean_pred || !d_f0_std_pred) return fail(DSD_ERR_INVALID, "dsf_cwt_pitch_loss_bwd: null argument");
    CwtLossParams p{};
    const int rc = cwt_loss_params(p, "dsf_cwt_pitch_loss_bwd", pred, sb, st, sc, cwt_spec, uv, mel2ph, f0_mean_pred, f0_mean, f0_std_pred, f0_std, B,
                                   T, channels, use_uv, l2, lam_f0, lam_uv);
    if (rc != DSD_OK) return rc;
    p.gout = grad_out; p.dpred = d_pred; p.dmean = d_f0_mean_pred; p.dstd = d_f0_std_pred;
    hipLaunchKernelGGL(k_cwt_loss_bwd, dim3((unsigned)std::min<long long>(1024, (p.n + kCwtBlock - 1) / kCwtBlock)), dim3(kCwtBlock), 0,
                       (hipStream_t)stream, p, stats);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
