// pe_train.hpp - what PitchExtractionTask (tasks/tts/pe.py) needs beyond the operators of fs2_kernels.hpp / fs2_train.hpp to TRAIN the
// PitchExtractor (modules/fastspeech/pe.py); C ABI in include/dsf.h ("PitchExtractor training").  Included at the end of dsd.hip (one
// translation unit: shares fail(), HIP_TRY, fs_ts()).
//
//   k_pe_bn_train        nn.BatchNorm1d on BATCH statistics (Prenet, pe.py:14-18 in train mode) with Prenet's ReLU in front (relu_in) and its
//                        `* nonpadding_mask` behind (pe.py:35): one workgroup per channel streams the B rows of the channel three times (sum,
//                        centred sum of squares, output; the first sum is taken relative to a pivot); up to 32 KB of a channel (8 x 1024 floats) stay in LDS between the passes.  The
//                        statistics run over the B * T live columns - padding frames count (F.batch_norm sees them), the TS - T tail never
//                        does.  Writes save_mean / save_rstd and updates running_mean / running_var (unbiased variance) in place.
//   k_pe_bn_train_bwd    dgamma, dbeta and dx = gamma rstd (g - mean(g) - xhat mean(g xhat)), g = dy * keep, times (pre > 0) under relu_in;
//                        one workgroup per channel, two passes.
//   k_pe_gn_bwd          backward of k_fs_group_norm (GroupNorm + ReLU; the residual's gradient is dy itself): one workgroup per (group,
//                        utterance) recomputes the mean (pivot + dm) / rstd with the forward's own loops (so the ReLU mask is the forward's, bit
//                        for bit), each wave sums the channels it owns (dgamma / dbeta partials of this utterance -> workspace), then dx.
//   k_pe_gn_reduce       dgamma[c] / dbeta[c] = the utterances' partials added in utterance order.
//   k_pe_f0_partial / k_pe_f0_final / k_pe_f0_bwd    FastSpeech2Task.add_f0_loss (tasks/tts/fs2.py:254-269) with the caller's nonpadding mask:
//                        uv = sum(BCEWithLogits(p1, uv) np) / sum(np) lambda_uv, f0 = sum(|p0 - f0| np') / sum(np') lambda_f0 (l2: the square),
//                        np' = np (uv == 0) under use_uv; BCE as max(x, 0) - x z + log1p(exp(-|x|)).
//
// fp32 throughout.  Every sum has a fixed order: two runs are bitwise equal.  No atomics.  The norms: per-thread strided sums, a shuffle tree
// per wave, the waves in order (fs_block_sum, fs2_kernels.hpp).  The f0 loss: per-thread strided sums, then block_sum's tree (block_sum.hpp),
// all four sums of a kernel in one call.
#pragma once
#include "block_sum.hpp"
#include "loss_math.hpp"

namespace dsd {

constexpr int kPeBnStage4 = 2048;        // float4s of one channel kept in LDS between the passes of k_pe_bn_train (32 KB)
constexpr int kPeGnMaxCg = 64;           // channels per group of k_pe_gn_bwd (GroupNorm(C / 16, C): 16)
constexpr int kPeF0Blocks = 256;         // partial blocks of the pitch loss

struct PeBnParams {
    const float* x;          // [B][C][TS] the convolution's output (pre-activation)
    const float* gamma;      // [C]
    const float* beta;       // [C]
    const float* keep;       // [B][T] or nullptr
    float* y;                // [B][C][TS]
    float* save_mean;        // [C]
    float* save_rstd;        // [C]
    float* run_mean;         // [C] or nullptr
    float* run_var;          // [C] or nullptr
    int B, C, T, TS;
    float eps, momentum;
    int relu_in;
};

__device__ __forceinline__ float4 pe_relu4(float4 v, int on) {
    return on ? make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)) : v;
}

__global__ __launch_bounds__(256) void k_pe_bn_train(const PeBnParams p) {
    __shared__ float4 stage[kPeBnStage4];
    __shared__ float red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int q = p.TS / 4, n4 = p.B * q;
    const bool staged = n4 <= kPeBnStage4;
    const float4* x4 = reinterpret_cast<const float4*>(p.x);
    // the sum is taken of x - pivot (pivot = the channel's first value): a mean far from zero keeps its digits (x = 100 +- 0.1)
    float pivot = p.x[(size_t)c * p.TS];
    if (p.relu_in) pivot = fmaxf(pivot, 0.f);
    float s = 0.f;
    for (int i = tid; i < n4; i += 256) {
        const int b = i / q, t4 = i - b * q, t = t4 * 4;
        const float4 v = pe_relu4(x4[((size_t)b * p.C + c) * q + t4], p.relu_in);
        if (staged) stage[i] = v;
        s += ((t < p.T ? v.x - pivot : 0.f) + (t + 1 < p.T ? v.y - pivot : 0.f)) + ((t + 2 < p.T ? v.z - pivot : 0.f) + (t + 3 < p.T ? v.w - pivot : 0.f));
    }
    const float n = (float)p.B * (float)p.T;
    const float mean = pivot + fs_block_sum(s, red) / n;
    float d = 0.f;
    for (int i = tid; i < n4; i += 256) {
        const int b = i / q, t4 = i - b * q, t = t4 * 4;
        const float4 v = staged ? stage[i] : pe_relu4(x4[((size_t)b * p.C + c) * q + t4], p.relu_in);
        const float e0 = t < p.T ? v.x - mean : 0.f, e1 = t + 1 < p.T ? v.y - mean : 0.f;
        const float e2 = t + 2 < p.T ? v.z - mean : 0.f, e3 = t + 3 < p.T ? v.w - mean : 0.f;
        d += (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
    }
    const float var = fs_block_sum(d, red) / n;
    const float rstd = 1.f / sqrtf(var + p.eps);
    if (tid == 0) {
        p.save_mean[c] = mean;
        p.save_rstd[c] = rstd;
        if (p.run_mean) p.run_mean[c] = (1.f - p.momentum) * p.run_mean[c] + p.momentum * mean;
        if (p.run_var) p.run_var[c] = (1.f - p.momentum) * p.run_var[c] + p.momentum * (var * (n / (n - 1.f)));
    }
    const float ga = p.gamma[c], be = p.beta[c];
    float4* y4 = reinterpret_cast<float4*>(p.y);
    for (int i = tid; i < n4; i += 256) {
        const int b = i / q, t4 = i - b * q, t = t4 * 4;
        const float4 v = staged ? stage[i] : pe_relu4(x4[((size_t)b * p.C + c) * q + t4], p.relu_in);
        const float r[4] = {v.x, v.y, v.z, v.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float w = 0.f;
            if (t + e < p.T) {
                w = (r[e] - mean) * rstd * ga + be;
                if (p.keep) w *= p.keep[(size_t)b * p.T + t + e];
            }
            o[e] = w;
        }
        y4[((size_t)b * p.C + c) * q + t4] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

struct PeBnBwdParams {
    const float* x;          // [B][C][TS] the forward's input (pre-activation)
    const float* dy;         // [B][C][TS]
    const float* gamma;      // [C]
    const float* keep;       // [B][T] or nullptr
    const float* save_mean;  // [C]
    const float* save_rstd;  // [C]
    float* dx;               // [B][C][TS]
    float* dgamma;           // [C]
    float* dbeta;            // [C]
    int B, C, T, TS;
    int relu_in;
};

__global__ __launch_bounds__(256) void k_pe_bn_train_bwd(const PeBnBwdParams p) {
    __shared__ float red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int q = p.TS / 4, n4 = p.B * q;
    const float4* x4 = reinterpret_cast<const float4*>(p.x);
    const float4* g4 = reinterpret_cast<const float4*>(p.dy);
    const float mean = p.save_mean[c], rstd = p.save_rstd[c];
    float s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < n4; i += 256) {
        const int b = i / q, t4 = i - b * q, t = t4 * 4;
        const size_t o = ((size_t)b * p.C + c) * q + t4;
        const float4 v = pe_relu4(x4[o], p.relu_in), gv = g4[o];
        const float r[4] = {v.x, v.y, v.z, v.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (t + e < p.T) {
                float g = gg[e];
                if (p.keep) g *= p.keep[(size_t)b * p.T + t + e];
                s1 += g;
                s2 += g * ((r[e] - mean) * rstd);
            }
        }
    }
    s1 = fs_block_sum(s1, red);
    s2 = fs_block_sum(s2, red);
    if (tid == 0) { p.dbeta[c] = s1; p.dgamma[c] = s2; }
    const float n = (float)p.B * (float)p.T;
    const float m1 = s1 / n, m2 = s2 / n, gr = p.gamma[c] * rstd;
    float4* d4 = reinterpret_cast<float4*>(p.dx);
    for (int i = tid; i < n4; i += 256) {
        const int b = i / q, t4 = i - b * q, t = t4 * 4;
        const size_t o = ((size_t)b * p.C + c) * q + t4;
        const float4 pre = x4[o], gv = g4[o];
        const float pr[4] = {pre.x, pre.y, pre.z, pre.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
        float out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float w = 0.f;
            if (t + e < p.T) {
                float g = gg[e];
                if (p.keep) g *= p.keep[(size_t)b * p.T + t + e];
                const float r = p.relu_in ? fmaxf(pr[e], 0.f) : pr[e];
                w = gr * (g - m1 - ((r - mean) * rstd) * m2);
                if (p.relu_in && !(pr[e] > 0.f)) w = 0.f;
            }
            out[e] = w;
        }
        d4[o] = make_float4(out[0], out[1], out[2], out[3]);
    }
}

// Backward of k_fs_group_norm: y = res + relu(xhat gamma + beta).  ws: [B][2][C] partials of dgamma / dbeta of utterance b.
__global__ __launch_bounds__(256) void k_pe_gn_bwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* __restrict__ dy, float* __restrict__ dx, float* __restrict__ ws, int C, int G, int T,
                                                  int TS, float eps, int relu) {
    __shared__ float red[4];
    __shared__ float chs[2][kPeGnMaxCg];
    const int g = blockIdx.x, bb = blockIdx.y, tid = threadIdx.x;
    const int cg = C / G;
    const size_t base = ((size_t)bb * C + (size_t)g * cg) * TS;
    const int n = cg * T;
    // pivot + dm / rstd: the loops of k_fs_group_norm, so that the ReLU mask below is the forward's
    const float pivot = x[base];
    float s = 0.f;
    for (int i = tid; i < n; i += 256) { const int c = i / T, t = i - c * T; s += x[base + (size_t)c * TS + t] - pivot; }
    const float dm = fs_block_sum(s, red) / (float)n;
    float d = 0.f;
    for (int i = tid; i < n; i += 256) { const int c = i / T, t = i - c * T; const float e = (x[base + (size_t)c * TS + t] - pivot) - dm; d += e * e; }
    const float var = fs_block_sum(d, red) / (float)n;
    const float rstd = 1.f / sqrtf(var + eps);
    // wave w owns channels w, w + 4, ...: sum over the frames of gz = dy * (z > 0) and of gz * xhat
    const int wave = tid >> 6, lane = tid & 63;
    for (int c = wave; c < cg; c += 4) {
        const int ch = g * cg + c;
        const float ga = gamma[ch], be = beta[ch];
        float a = 0.f, b = 0.f;
        for (int t = lane; t < T; t += 64) {
            const size_t o = base + (size_t)c * TS + t;
            const float xh = ((x[o] - pivot) - dm) * rstd;
            float gz = dy[o];
            if (relu && !(xh * ga + be > 0.f)) gz = 0.f;
            a += gz * xh;
            b += gz;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
        if (lane == 0) {
            chs[0][c] = a; chs[1][c] = b;
            ws[((size_t)bb * 2 + 0) * C + ch] = a;
            ws[((size_t)bb * 2 + 1) * C + ch] = b;
        }
    }
    __syncthreads();
    float s1 = 0.f, s2 = 0.f;                // sums over the group of gz gamma and gz gamma xhat
    for (int c = 0; c < cg; ++c) { const float ga = gamma[g * cg + c]; s1 += ga * chs[1][c]; s2 += ga * chs[0][c]; }
    const float m1 = s1 / (float)n, m2 = s2 / (float)n;
    const int nn = cg * TS;
    for (int i = tid; i < nn; i += 256) {
        const int c = i / TS, t = i - c * TS;
        const size_t o = base + (size_t)c * TS + t;
        float v = 0.f;
        if (t < T) {
            const int ch = g * cg + c;
            const float ga = gamma[ch];
            const float xh = ((x[o] - pivot) - dm) * rstd;
            float gz = dy[o];
            if (relu && !(xh * ga + beta[ch] > 0.f)) gz = 0.f;
            v = rstd * (gz * ga - m1 - xh * m2);
        }
        dx[o] = v;
    }
}

__global__ __launch_bounds__(256) void k_pe_gn_reduce(const float* __restrict__ ws, float* __restrict__ dgamma, float* __restrict__ dbeta, int B, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, b = 0.f;
    for (int r = 0; r < B; ++r) { a += ws[((size_t)r * 2 + 0) * C + c]; b += ws[((size_t)r * 2 + 1) * C + c]; }
    dgamma[c] = a;
    dbeta[c] = b;
}

struct PeF0Params {
    const float* pred;       // [B][T][Cp], element strides sb / st / sc
    long long sb, st, sc;
    const float* f0;         // [B][T]
    const float* uv;         // [B][T] (use_uv) or nullptr
    const float* np;         // [B][T] nonpadding
    float* partial;          // [nblk][4]
    float* out;              // [4]: uv loss, f0 loss, sum np, sum np'
    const float* gout;       // bwd: DEVICE [2], the upstream gradients of out[0], out[1]
    float* dpred;            // bwd: [B][T][Cp] contiguous
    long long n;             // B * T
    int T, Cp, nblk, use_uv, l2;
    float lam_uv, lam_f0;
};

__global__ __launch_bounds__(256) void k_pe_f0_partial(const PeF0Params p) {
    float a_uv = 0.f, a_np = 0.f, a_f0 = 0.f, a_npv = 0.f;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < p.n; i += (long long)gridDim.x * 256) {
        const long long b = i / p.T, t = i - b * p.T;
        const float* pr = p.pred + b * p.sb + t * p.st;
        float w = p.np[i];
        if (p.use_uv) {
            const float xl = pr[p.sc], z = p.uv[i];
            a_uv += bce_logits(xl, z) * w;
            a_np += w;
            w = w * (z == 0.f ? 1.f : 0.f);
        }
        const float df = pr[0] - p.f0[i];
        a_f0 += (p.l2 ? df * df : fabsf(df)) * w;
        a_npv += w;
    }
    float tot[4] = {a_uv, a_np, a_f0, a_npv};
    block_sum(tot);
    if (threadIdx.x == 0) {
        float* o = p.partial + (size_t)blockIdx.x * 4;
        o[0] = tot[0]; o[1] = tot[1]; o[2] = tot[2]; o[3] = tot[3];
    }
}

__global__ __launch_bounds__(256) void k_pe_f0_final(const PeF0Params p) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < p.nblk; i += 256) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += p.partial[(size_t)i * 4 + k];
    }
    block_sum(a);
    const float t0 = a[0], t1 = a[1], t2 = a[2], t3 = a[3];
    if (threadIdx.x == 0) {
        p.out[0] = p.use_uv ? t0 / t1 * p.lam_uv : 0.f;
        p.out[1] = t2 / t3 * p.lam_f0;
        p.out[2] = t1;
        p.out[3] = t3;
    }
}

// d pitch_pred of gout[0] out[0] + gout[1] out[1]; stats = the forward's out (the two mask sums)
__global__ __launch_bounds__(256) void k_pe_f0_bwd(const PeF0Params p, const float* __restrict__ stats) {
    const float c_uv = p.use_uv ? p.gout[0] * p.lam_uv / stats[2] : 0.f;
    const float c_f0 = p.gout[1] * p.lam_f0 / stats[3];
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < p.n; i += (long long)gridDim.x * 256) {
        const long long b = i / p.T, t = i - b * p.T;
        const float* pr = p.pred + b * p.sb + t * p.st;
        float* dp = p.dpred + i * p.Cp;
        float w = p.np[i];
        for (int k = 1; k < p.Cp; ++k) dp[k] = 0.f;
        if (p.use_uv) {
            const float xl = pr[p.sc], z = p.uv[i];
            dp[1] = c_uv * (w * bce_logits_grad(xl, z));
            w = w * (z == 0.f ? 1.f : 0.f);
        }
        const float df = pr[0] - p.f0[i];
        const float dd = p.l2 ? 2.f * df : loss_sign(df);
        dp[0] = c_f0 * (w * dd);
    }
}

}  // namespace dsd

// ------------------------------------------------------------------------------------------------------------
// host side (C ABI in include/dsf.h)
// ------------------------------------------------------------------------------------------------------------
extern "C" int dsf_batch_norm_train(const float* x, const float* gamma, const float* beta, const float* keep, float* y, float* save_mean,
                                    float* save_rstd, float* running_mean, float* running_var, int32_t B, int32_t C, int32_t T, float eps,
                                    float momentum, int32_t relu_in, void* stream) {
    if (!x || !gamma || !beta || !y || !save_mean || !save_rstd) return fail(DSD_ERR_INVALID, "dsf_batch_norm_train: null argument");
    if (B < 1 || C < 1 || C > 65535 || T < 1 || (int64_t)B * fs_ts(T) / 4 > INT32_MAX)
        return fail(DSD_ERR_INVALID, "dsf_batch_norm_train: bad shape (B=%d C=%d T=%d)", B, C, T);
    if ((int64_t)B * T < 2) return fail(DSD_ERR_INVALID, "dsf_batch_norm_train: batch statistics need more than one value per channel (B * T = %d)", B * T);
    PeBnParams p{};
    p.x = x; p.gamma = gamma; p.beta = beta; p.keep = keep; p.y = y; p.save_mean = save_mean; p.save_rstd = save_rstd;
    p.run_mean = running_mean; p.run_var = running_var; p.B = B; p.C = C; p.T = T; p.TS = fs_ts(T); p.eps = eps; p.momentum = momentum;
    p.relu_in = relu_in;
    hipLaunchKernelGGL(k_pe_bn_train, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_batch_norm_train_bwd(const float* x, const float* save_mean, const float* save_rstd, const float* gamma, const float* dy,
                                        const float* keep, float* dx, float* dgamma, float* dbeta, int32_t B, int32_t C, int32_t T,
                                        int32_t relu_in, void* stream) {
    if (!x || !save_mean || !save_rstd || !gamma || !dy || !dx || !dgamma || !dbeta)
        return fail(DSD_ERR_INVALID, "dsf_batch_norm_train_bwd: null argument");
    if (B < 1 || C < 1 || C > 65535 || T < 1 || (int64_t)B * fs_ts(T) / 4 > INT32_MAX)
        return fail(DSD_ERR_INVALID, "dsf_batch_norm_train_bwd: bad shape (B=%d C=%d T=%d)", B, C, T);
    if ((int64_t)B * T < 2) return fail(DSD_ERR_INVALID, "dsf_batch_norm_train_bwd: batch statistics need more than one value per channel (B * T = %d)", B * T);
    PeBnBwdParams p{};
    p.x = x; p.dy = dy; p.gamma = gamma; p.keep = keep; p.save_mean = save_mean; p.save_rstd = save_rstd; p.dx = dx; p.dgamma = dgamma;
    p.dbeta = dbeta; p.B = B; p.C = C; p.T = T; p.TS = fs_ts(T); p.relu_in = relu_in;
    hipLaunchKernelGGL(k_pe_bn_train_bwd, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsf_group_norm_bwd_workspace_floats(int32_t B, int32_t C) {
    if (B < 1 || C < 1) return -1;
    return (int64_t)B * 2 * C;
}

extern "C" int dsf_group_norm_bwd(const float* x, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma, float* dbeta,
                                  float* workspace, int32_t B, int32_t C, int32_t groups, int32_t T, float eps, int32_t relu, void* stream) {
    if (!x || !gamma || !beta || !dy || !dx || !dgamma || !dbeta || !workspace) return fail(DSD_ERR_INVALID, "dsf_group_norm_bwd: null argument");
    if (B < 1 || B > 65535 || C < 1 || groups < 1 || (C % groups) || C / groups > kPeGnMaxCg || T < 1)
        return fail(DSD_ERR_INVALID, "dsf_group_norm_bwd: bad shape (B=%d C=%d groups=%d T=%d; at most %d channels per group)", B, C, groups, T,
                    kPeGnMaxCg);
    hipLaunchKernelGGL(k_pe_gn_bwd, dim3((unsigned)groups, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, dy, dx, workspace, C,
                       groups, T, fs_ts(T), eps, relu);
    hipLaunchKernelGGL(k_pe_gn_reduce, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dgamma, dbeta, B, C);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsf_f0_loss_workspace_floats(void) { return (int64_t)kPeF0Blocks * 4; }

static int pe_f0_params(PeF0Params& p, const char* what, const float* pred, int64_t sb, int64_t st, int64_t sc, const float* f0, const float* uv,
                        const float* nonpadding, int32_t B, int32_t T, int32_t Cp, int32_t use_uv, int32_t l2, float lam_uv, float lam_f0) {
    if (!pred || !f0 || !nonpadding || (use_uv && !uv)) return fail(DSD_ERR_INVALID, "%s: null argument", what);
    if (B < 1 || T < 1 || Cp < (use_uv ? 2 : 1)) return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d T=%d channels=%d use_uv=%d)", what, B, T, Cp, use_uv);
    p.pred = pred; p.sb = sb; p.st = st; p.sc = sc; p.f0 = f0; p.uv = use_uv ? uv : nullptr; p.np = nonpadding; p.n = (long long)B * T; p.T = T;
    p.Cp = Cp; p.use_uv = use_uv ? 1 : 0; p.l2 = l2 ? 1 : 0; p.lam_uv = lam_uv; p.lam_f0 = lam_f0;
    p.nblk = (int)std::min<long long>(kPeF0Blocks, (p.n + 255) / 256);
    return DSD_OK;
}

extern "C" int dsf_f0_loss(const float* pitch_pred, int64_t sb, int64_t st, int64_t sc, const float* f0, const float* uv, const float* nonpadding,
                           int32_t B, int32_t T, int32_t channels, int32_t use_uv, int32_t l2, float lam_uv, float lam_f0, float* workspace,
                           float* out, void* stream) {
    if (!workspace || !out) return fail(DSD_ERR_INVALID, "dsf_f0_loss: null argument");
    PeF0Params p{};
    const int rc = pe_f0_params(p, "dsf_f0_loss", pitch_pred, sb, st, sc, f0, uv, nonpadding, B, T, channels, use_uv, l2, lam_uv, lam_f0);
    if (rc != DSD_OK) return rc;
    p.partial = workspace; p.out = out;
    hipLaunchKernelGGL(k_pe_f0_partial, dim3((unsigned)p.nblk), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(k_pe_f0_final, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsf_f0_loss_bwd(const float* pitch_pred, int64_t sb, int64_t st, int64_t sc, const float* f0, const float* uv, const float* nonpadding,
                               int32_t B, int32_t T, int32_t channels, int32_t use_uv, int32_t l2, float lam_uv, float lam_f0, const float* stats,
                               const float* grad_out, float* d_pitch_pred, void* stream) {
    if (!stats || !grad_out || !d_pitch_pred) return fail(DSD_ERR_INVALID, "dsf_f0_loss_bwd: null argument");
    PeF0Params p{};
    const int rc = pe_f0_params(p, "dsf_f0_loss_bwd", pitch_pred, sb, st, sc, f0, uv, nonpadding, B, T, channels, use_uv, l2, lam_uv, lam_f0);
    if (rc != DSD_OK) return rc;
    p.gout = grad_out; p.dpred = d_pitch_pred;
    hipLaunchKernelGGL(k_pe_f0_bwd, dim3((unsigned)std::min<long long>(1024, (p.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, stats);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
