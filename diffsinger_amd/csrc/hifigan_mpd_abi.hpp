// hifigan_mpd_abi.hpp - host side of the HiFi-GAN period discriminator (C ABI in include/dsv.h, section "HiFi-GAN period discriminator"; kernels in
// hifigan_mpd.hpp); included at the end of dsd.hip.  Every entry point validates on the host and refuses with DSD_ERR_INVALID before any launch;
// nothing allocates, synchronises or reads a device value.
#include "hifigan_mpd.hpp"
#include "voc_train_host.hpp"

static int hgp_out_h(int H, int S) { return (H - 1) / S + 1; }       // K = 5, padding 2

extern "C" int32_t dsv_hgp_height(int32_t H, int32_t stride) { return (H < 1 || stride < 1) ? -1 : hgp_out_h(H, stride); }

// samples after the reflect pad to a multiple of the period; -1 where the pad would not be shorter than the signal (F.pad refuses it too)
extern "C" int64_t dsv_hgp_folded_samples(int32_t T, int32_t period) {
    if (T < 1 || period < 1 || period > 64) return -1;
    const int64_t Tp = ((int64_t)T + period - 1) / period * period;
    return Tp - T >= T ? -1 : Tp;
}

static int hgp_check_stride(const char* who, int S) {
    if (S != 1 && S != 3) return fail(DSD_ERR_INVALID, "%s: stride=%d must be 1 or 3", who, S);
    return DSD_OK;
}
static int hgp_check_channels(const char* who, int Ci, int Co) {
    if (Ci < 32 || Co < 32 || Ci % 32 || Co % 32 || Ci > 4096 || Co > 4096)
        return fail(DSD_ERR_INVALID, "%s: Ci=%d and Co=%d must be multiples of 32 in [32, 4096]", who, Ci, Co);
    return DSD_OK;
}

extern "C" int dsv_hgp_fold(const float* x, float* out, int32_t B, int32_t T, int64_t ld_x, int32_t period, void* stream) {
    if (!x || !out) return fail(DSD_ERR_INVALID, "dsv_hgp_fold: null argument");
    const int64_t Tp = dsv_hgp_folded_samples(T, period);
    if (Tp < 0) return fail(DSD_ERR_INVALID, "dsv_hgp_fold: T=%d, period=%d: the reflect pad must be shorter than the signal (period in [1, 64])", T, period);
    DSD_TRY(voc_check_period_shape("dsv_hgp_fold", B, (int)(Tp / period), period));
    DSD_TRY(voc_check_row_stride("dsv_hgp_fold", ld_x, T));
    DSD_TRY(voc_check_disjoint("dsv_hgp_fold", x, (B - 1) * ld_x + T, out, (int64_t)B * Tp));
    hipLaunchKernelGGL(k_hgp_fold, dim3((unsigned)((Tp + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, out, T, (long long)ld_x, (int)Tp);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_fold_backward(const float* g, float* dx, int32_t B, int32_t T, int32_t period, void* stream) {
    if (!g || !dx) return fail(DSD_ERR_INVALID, "dsv_hgp_fold_backward: null argument");
    const int64_t Tp = dsv_hgp_folded_samples(T, period);
    if (Tp < 0)
        return fail(DSD_ERR_INVALID, "dsv_hgp_fold_backward: T=%d, period=%d: the reflect pad must be shorter than the signal (period in [1, 64])", T, period);
    DSD_TRY(voc_check_period_shape("dsv_hgp_fold_backward", B, (int)(Tp / period), period));
    DSD_TRY(voc_check_disjoint("dsv_hgp_fold_backward", g, (int64_t)B * Tp, dx, (int64_t)B * T));
    hipLaunchKernelGGL(k_hgp_fold_bwd, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, dx, T, (int)Tp);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

// ---- edge layers ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t dsv_hgp_edge_workspace_floats(int32_t B, int32_t H, int32_t period, int32_t C, int32_t K) {
    if (!voc_period_shape_ok(B, H, period) || C < 1 || C > 65535 || K < 1 || K > kHgpK) return -1;
    return (int64_t)voc_splits(B * H * period, kHgpEdgeSplit) * C * (K + 1);
}

static int hgp_edge_grad(const char* who, const float* P, const float* P2, const float* Q, float* ws, float* dw, float* db, int C, int KT, int pad, int S,
                         int B, int Hp, int Hq, int p, size_t bs_p, size_t cs_p, size_t bs_q, size_t cs_q, int per_channel_bias, hipStream_t s) {
    const int nsplit = voc_splits(B * Hp * p, kHgpEdgeSplit);
    if (nsplit > 65535) return fail(DSD_ERR_INVALID, "%s: %d splits exceed 65535 workgroups", who, nsplit);
    hipLaunchKernelGGL(k_hgp_edge_wgrad, dim3((unsigned)C, (unsigned)nsplit), dim3(256), 0, s, P, P2, Q, ws, C, KT, pad, S, Hp, Hq, p,
                       (long long)B * Hp * p, bs_p, cs_p, bs_q, cs_q);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_hgp_edge_reduce, dim3((unsigned)((C * (KT + 1) + 255) / 256)), dim3(256), 0, s, (const float*)ws, dw, db, nsplit, C, KT,
                       per_channel_bias);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_first(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t H, int32_t period,
                             int32_t stride, float slope, void* stream) {
    if (!x || !w || !out) return fail(DSD_ERR_INVALID, "dsv_hgp_first: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_first", B, H, period));
    DSD_TRY(hgp_check_stride("dsv_hgp_first", stride));
    DSD_TRY(voc_check_slope("dsv_hgp_first", slope));
    DSD_TRY(voc_check_grid_channels("dsv_hgp_first", C));
    const int Ho = hgp_out_h(H, stride);
    DSD_TRY(voc_check_disjoint("dsv_hgp_first", x, (int64_t)B * H * period, out, (int64_t)B * C * Ho * period));
    hipLaunchKernelGGL(k_hgp_first, dim3((unsigned)((Ho * period + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, w, bias, out,
                       C, H, Ho, period, stride, slope);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_first_backward(const float* g0, const float* x, const float* w, float* workspace, float* dw, float* db, float* dx, int32_t B,
                                      int32_t C, int32_t H, int32_t period, int32_t stride, void* stream) {
    if (!g0 || !x || !w || !workspace || !dw) return fail(DSD_ERR_INVALID, "dsv_hgp_first_backward: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_first_backward", B, H, period));
    DSD_TRY(hgp_check_stride("dsv_hgp_first_backward", stride));
    DSD_TRY(voc_check_grid_channels("dsv_hgp_first_backward", C));
    const int Ho = hgp_out_h(H, stride);
    const size_t gplane = (size_t)Ho * period;
    DSD_TRY(hgp_edge_grad("dsv_hgp_first_backward", g0, nullptr, x, workspace, dw, db, C, kHgpK, kHgpPad, stride, B, Ho, H, period, (size_t)C * gplane, gplane,
                          (size_t)H * period, 0, 1, (hipStream_t)stream));
    if (dx) {
        DSD_TRY(voc_check_disjoint("dsv_hgp_first_backward", g0, (int64_t)B * C * gplane, dx, (int64_t)B * H * period));
        hipLaunchKernelGGL(k_hgp_first_dx, dim3((unsigned)((H * period + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g0, w, dx, C, H, Ho,
                           period, stride);
        HIP_TRY(hipGetLastError());
    }
    return DSD_OK;
}

extern "C" int dsv_hgp_post(const float* a, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t H, int32_t period, void* stream) {
    if (!a || !w || !out) return fail(DSD_ERR_INVALID, "dsv_hgp_post: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_post", B, H, period));
    DSD_TRY(voc_check_grid_channels("dsv_hgp_post", C));
    DSD_TRY(voc_check_disjoint("dsv_hgp_post", a, (int64_t)B * C * H * period, out, (int64_t)B * H * period));
    hipLaunchKernelGGL(k_hgp_post, dim3((unsigned)((H * period + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a, w, bias, out, C, H, period);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_post_backward(const float* gp, const float* gp2, const float* a, const float* w, const float* cot, float* workspace, float* dw,
                                     float* db, float* ga, int32_t B, int32_t C, int32_t H, int32_t period, float slope, void* stream) {
    if (!gp || !a || !w || !workspace || !dw || !ga) return fail(DSD_ERR_INVALID, "dsv_hgp_post_backward: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_post_backward", B, H, period));
    DSD_TRY(voc_check_slope("dsv_hgp_post_backward", slope));
    DSD_TRY(voc_check_grid_channels("dsv_hgp_post_backward", C));
    const size_t plane = (size_t)H * period;
    DSD_TRY(voc_check_disjoint("dsv_hgp_post_backward", a, (int64_t)B * C * plane, ga, (int64_t)B * C * plane));
    DSD_TRY(hgp_edge_grad("dsv_hgp_post_backward", gp, gp2, a, workspace, dw, db, C, kHgpPostK, 1, 1, B, H, H, period, plane, 0, (size_t)C * plane, plane, 0,
                          (hipStream_t)stream));
    hipLaunchKernelGGL(k_hgp_post_dgrad, dim3((unsigned)((plane + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0, (hipStream_t)stream, gp, gp2, a, w, cot,
                       ga, C, H, period, slope);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

// ---- dense layers ---------------------------------------------------------------------------------------------------------------------------------
// taps of input phase r of the data gradient, as a bit mask: k with (r + 2 - k) mod S = 0
static int hgp_phase_taps(int S, int r) {
    int m = 0;
    for (int k = 0; k < kHgpK; ++k)
        if (((r + kHgpPad - k) % S + S) % S == 0) m |= 1 << k;
    return m;
}
extern "C" int32_t dsv_hgp_dgrad_phase_taps(int32_t stride, int32_t phase) {
    if ((stride != 1 && stride != 3) || phase < 0 || phase >= stride) return -1;
    return hgp_phase_taps(stride, phase);
}
// float offset of phase `phase`'s packed matrix ([Ci][Co][taps of the phase] through dsv_pack_weight) in the data gradient's weight buffer;
// phase = stride: the buffer's size
extern "C" int64_t dsv_hgp_dgrad_packed_offset(int32_t Ci, int32_t Co, int32_t stride, int32_t phase) {
    if ((stride != 1 && stride != 3) || phase < 0 || phase > stride || Ci < 32 || Co < 32 || Ci % 32 || Co % 32) return -1;
    int64_t off = 0;
    for (int r = 0; r < phase; ++r) off += dsv_packed_floats(Ci, Co, __builtin_popcount(hgp_phase_taps(stride, r)));
    return off;
}

static int hgp_launch_gemm(const HgpGemmParams& p, int64_t max_cols, hipStream_t s, int nph) {
    const dim3 grid((unsigned)((max_cols + kHgpTileN - 1) / kHgpTileN), (unsigned)((p.Cdst + kHgpTileM - 1) / kHgpTileM), (unsigned)nph);
    hipLaunchKernelGGL(k_hgp_gemm, grid, dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_conv(const float* x, const float* w_packed, const float* bias, float* out, int32_t B, int32_t Ci, int32_t Co, int32_t H,
                            int32_t period, int32_t stride, float slope, void* stream) {
    if (!x || !w_packed || !out) return fail(DSD_ERR_INVALID, "dsv_hgp_conv: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_conv", B, H, period));
    DSD_TRY(hgp_check_channels("dsv_hgp_conv", Ci, Co));
    DSD_TRY(hgp_check_stride("dsv_hgp_conv", stride));
    DSD_TRY(voc_check_slope("dsv_hgp_conv", slope));
    const int Ho = hgp_out_h(H, stride);
    DSD_TRY(voc_check_disjoint("dsv_hgp_conv", x, (int64_t)B * Ci * H * period, out, (int64_t)B * Co * Ho * period));
    HgpGemmParams p{};
    p.src = x; p.bias = bias; p.dst = out;
    p.B = B; p.Csrc = Ci; p.Hsrc = H; p.Cdst = Co; p.Hdst = Ho; p.p = period; p.S = stride; p.So = 1; p.slope = slope; p.bwd = 0;
    p.ph[0].wp = reinterpret_cast<const float4*>(w_packed); p.ph[0].KT = kHgpK; p.ph[0].cols_h = Ho; p.ph[0].ro = 0;
    for (int k = 0; k < kHgpK; ++k) p.ph[0].e[k] = k - kHgpPad;
    return hgp_launch_gemm(p, (int64_t)B * Ho * period, (hipStream_t)stream, 1);
}

extern "C" int dsv_hgp_conv_dgrad(const float* g, const float* w_packed, const float* cot, const float* saved, float* out, int32_t B, int32_t Ci,
                                  int32_t Co, int32_t H, int32_t period, int32_t stride, float slope, void* stream) {
    if (!g || !w_packed || !out) return fail(DSD_ERR_INVALID, "dsv_hgp_conv_dgrad: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_conv_dgrad", B, H, period));
    DSD_TRY(hgp_check_channels("dsv_hgp_conv_dgrad", Ci, Co));
    DSD_TRY(hgp_check_stride("dsv_hgp_conv_dgrad", stride));
    DSD_TRY(voc_check_slope("dsv_hgp_conv_dgrad", slope));
    const int Ho = hgp_out_h(H, stride);
    DSD_TRY(voc_check_disjoint("dsv_hgp_conv_dgrad", g, (int64_t)B * Co * Ho * period, out, (int64_t)B * Ci * H * period));
    HgpGemmParams p{};
    p.src = g; p.cot = cot; p.saved = saved; p.dst = out;
    p.B = B; p.Csrc = Co; p.Hsrc = Ho; p.Cdst = Ci; p.Hdst = H; p.p = period; p.S = 1; p.So = stride; p.slope = slope; p.bwd = 1;
    int64_t max_cols = 0;
    for (int r = 0; r < stride; ++r) {
        HgpPhase& ph = p.ph[r];
        ph.wp = reinterpret_cast<const float4*>(w_packed + dsv_hgp_dgrad_packed_offset(Ci, Co, stride, r));
        const int taps = hgp_phase_taps(stride, r);
        ph.KT = 0;
        for (int k = 0; k < kHgpK; ++k)
            if (taps >> k & 1) ph.e[ph.KT++] = (r + kHgpPad - k) / stride;
        ph.cols_h = H > r ? (H - r + stride - 1) / stride : 0;       // input rows S m + r < H
        ph.ro = r;
        max_cols = std::max(max_cols, (int64_t)B * ph.cols_h * period);
    }
    return hgp_launch_gemm(p, max_cols, (hipStream_t)stream, stride);
}

// splits of the position axis of the weight gradient: none where the output tiles alone fill the chip's 256 compute units (the 1024 -> 1024
// layer: 256 workgroups over a few thousand positions) or the positions fit one split; else kSplitK positions each (512 -> 1024 has 128 tiles:
// unsplit it ran at half the rate of the 1024 -> 1024 layer, 0.39 ms against 0.38 ms for half the work)
static int hgp_wgrad_splits(int64_t npos, int Ci, int Co) {
    const int tiles = ((Co + kHgpWgM - 1) / kHgpWgM) * (Ci / kHgpWgN);
    if (tiles >= 256 || npos <= kSplitK) return 1;
    return (int)((npos + kSplitK - 1) / kSplitK);
}
extern "C" int32_t dsv_hgp_wgrad_splits(int32_t B, int32_t Ci, int32_t Co, int32_t H_out, int32_t period) {
    if (!voc_period_shape_ok(B, H_out, period) || Ci < 32 || Co < 32 || Ci % 32 || Co % 32) return -1;
    return hgp_wgrad_splits((int64_t)B * H_out * period, Ci, Co);
}
extern "C" int64_t dsv_hgp_wgrad_workspace_floats(int32_t B, int32_t Ci, int32_t Co, int32_t H_out, int32_t period) {
    const int n = dsv_hgp_wgrad_splits(B, Ci, Co, H_out, period);
    if (n < 0) return -1;
    return n == 1 ? 0 : (int64_t)n * Co * Ci * kHgpK;
}

extern "C" int dsv_hgp_conv_wgrad(const float* g, const float* x, float* workspace, float* dw, float* db, int32_t B, int32_t Ci, int32_t Co, int32_t H,
                                  int32_t period, int32_t stride, void* stream) {
    if (!g || !x || !dw) return fail(DSD_ERR_INVALID, "dsv_hgp_conv_wgrad: null argument");
    DSD_TRY(voc_check_period_shape("dsv_hgp_conv_wgrad", B, H, period));
    DSD_TRY(hgp_check_channels("dsv_hgp_conv_wgrad", Ci, Co));
    DSD_TRY(hgp_check_stride("dsv_hgp_conv_wgrad", stride));
    const int Ho = hgp_out_h(H, stride);
    const int64_t npos = (int64_t)B * Ho * period;
    const int nsplit = hgp_wgrad_splits(npos, Ci, Co);
    if (nsplit > 1 && !workspace) return fail(DSD_ERR_INVALID, "dsv_hgp_conv_wgrad: %d splits need the workspace", nsplit);
    if (nsplit > 65535) return fail(DSD_ERR_INVALID, "dsv_hgp_conv_wgrad: %d splits exceed 65535 workgroups", nsplit);
    const int n = Co * Ci * kHgpK;
    HgpWgradParams p{};
    p.g = g; p.x = x; p.out = nsplit > 1 ? workspace : dw;
    p.B = B; p.Co = Co; p.Ci = Ci; p.Hout = Ho; p.Hin = H; p.p = period; p.S = stride;
    p.npos = npos; p.chunk = nsplit > 1 ? kSplitK : (npos + 31) / 32 * 32;
    hipLaunchKernelGGL(k_hgp_wgrad, dim3((unsigned)((Co + kHgpWgM - 1) / kHgpWgM), (unsigned)(Ci / kHgpWgN), (unsigned)nsplit), dim3(kThreads), 0,
                       (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    if (nsplit > 1) {
        hipLaunchKernelGGL(k_split_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, n, nsplit);
        HIP_TRY(hipGetLastError());
    }
    if (db) {
        hipLaunchKernelGGL(k_hgp_bias_grad, dim3((unsigned)Co), dim3(256), 0, (hipStream_t)stream, g, db, B, Co, Ho * period);
        HIP_TRY(hipGetLastError());
    }
    return DSD_OK;
}

// ---- feature-matching L1 ------------------------------------------------------------------------------------------------------------------------------
static int hgp_l1_blocks(int64_t n) {
    const int64_t want = (n + 4 * kHgpLossThreads - 1) / (4 * kHgpLossThreads);
    return (int)(want < 1 ? 1 : want > kHgpLossMaxBlocks ? kHgpLossMaxBlocks : want);
}
// float64 partial sums one pair of n elements writes (dsv_hgp_l1_partial); -1 for a bad n
extern "C" int32_t dsv_hgp_l1_blocks(int64_t n) { return (n < 1 || n > ((int64_t)1 << 40)) ? -1 : hgp_l1_blocks(n); }

extern "C" int dsv_hgp_l1_partial(const float* r, const float* g, void* workspace, int64_t n, void* stream) {
    if (!r || !g || !workspace) return fail(DSD_ERR_INVALID, "dsv_hgp_l1_partial: null argument");
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(DSD_ERR_INVALID, "dsv_hgp_l1_partial: bad shape (n=%lld must be in [1, 2^40])", (long long)n);
    DSD_TRY(voc_check_f64_workspace("dsv_hgp_l1_partial", workspace, "it holds float64 sums"));
    hipLaunchKernelGGL(k_hgp_l1_partial, dim3((unsigned)hgp_l1_blocks(n)), dim3(kHgpLossThreads), 0, (hipStream_t)stream, r, g, (double*)workspace,
                       (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_l1_final(const void* workspace, int32_t nblocks, float* out, void* stream) {
    if (!workspace || !out) return fail(DSD_ERR_INVALID, "dsv_hgp_l1_final: null argument");
    if (nblocks < 1) return fail(DSD_ERR_INVALID, "dsv_hgp_l1_final: bad shape (nblocks=%d must be >= 1)", nblocks);
    DSD_TRY(voc_check_f64_workspace("dsv_hgp_l1_final", workspace, "it holds float64 sums"));
    hipLaunchKernelGGL(k_hgp_l1_final, dim3(1), dim3(kHgpLossThreads), 0, (hipStream_t)stream, (const double*)workspace, out, nblocks);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgp_l1_backward(const float* r, const float* g, const float* grad_out, float* dr, float* dg, int64_t n, void* stream) {
    if (!r || !g || !grad_out || !dr || !dg) return fail(DSD_ERR_INVALID, "dsv_hgp_l1_backward: null argument");
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(DSD_ERR_INVALID, "dsv_hgp_l1_backward: bad shape (n=%lld must be in [1, 2^40])", (long long)n);
    const int64_t want = (n + kHgpLossThreads - 1) / kHgpLossThreads;
    hipLaunchKernelGGL(k_hgp_l1_bwd, dim3((unsigned)(want > 16384 ? 16384 : want)), dim3(kHgpLossThreads), 0, (hipStream_t)stream, r, g, grad_out, dr, dg,
                       (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
