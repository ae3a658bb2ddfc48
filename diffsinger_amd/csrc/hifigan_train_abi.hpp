// hifigan_train_abi.hpp - host side of HiFi-GAN generator training (C ABI in include/dsv.h, section "HiFi-GAN generator training"; kernels in
// hifigan_train.hpp); included at the end of dsd.hip behind pwg_train_abi.hpp.  Every entry point validates on the host and refuses with
// DSD_ERR_INVALID before any launch; nothing allocates or synchronises; everything is enqueued on the caller's stream.  Every buffer length is
// one exported 64-bit function; an entry point that takes a workspace takes its length and refuses one shorter than its own requirement.
#include "hifigan_train.hpp"
#include "voc_train_host.hpp"

extern "C" int32_t dsv_hgt_wgrad_split(void) { return kSplitK; }

static bool hgt_ch_ok(int C) { return C >= 1 && C <= 1024; }
// taps of a convolution with kernel K, dilation dil, padding pad stay within +-kVocHaloWide samples, on both sides
static bool hgt_reach_ok(int K, int dil, int pad) {
    return K >= 1 && K <= 64 && dil >= 1 && dil <= 64 && pad >= 0 && pad <= kVocHaloWide && (K - 1) * dil - pad >= 0 && (K - 1) * dil - pad <= kVocHaloWide;
}

extern "C" int64_t dsv_hgt_act_floats(int32_t B, int32_t C, int32_t L) {
    if (!voc_shape_ok(B, L) || !hgt_ch_ok(C)) return -1;
    return (int64_t)B * C * voc_ls(L);
}

extern "C" int64_t dsv_hgt_wgrad_workspace_floats(int32_t B, int32_t L, int32_t Co, int32_t Ci, int32_t K, int32_t up) {
    if (!voc_shape_ok(B, L) || !hgt_ch_ok(Co) || !hgt_ch_ok(Ci) || K < 1 || K > 64 || up < 1 || up > 64 || (int64_t)L * up > (1 << 30)) return -1;
    return (int64_t)B * voc_splits(L, kSplitK) * ((int64_t)Co * up) * ((int64_t)Ci * K);
}

template <int NB, int WT, int HALO>
static void hgt_dgrad_launch(const HgtDgradParams& p, int B, hipStream_t s) {
    if (first_on_device(800 + 10 * NB + WT + 1000 * (HALO != kVocHalo))) {
        (void)hipFuncSetAttribute((const void*)k_hgt_dgrad<NB, WT, HALO>, hipFuncAttributeMaxDynamicSharedMemorySize, voc_lds_bytes<NB, WT, HALO>());
    }
    constexpr int WR = 4 / WT, SPAN = voc_span<NB, WT>();
    const dim3 grid((unsigned)((p.LS + SPAN - 1) / SPAN), (unsigned)B, (unsigned)((p.rows + 32 * WR - 1) / (32 * WR)));
    const size_t lds = (size_t)voc_lds_bytes<NB, WT, HALO>();
    hipLaunchKernelGGL((k_hgt_dgrad<NB, WT, HALO>), grid, dim3(kThreads), lds, s, p);
}

extern "C" int dsv_hgt_conv_dgrad(const float* g, const float* wt_packed, const float* x_saved, const float* residual, const float* sum_in, float* dx,
                                  int32_t B, int32_t Cg, int32_t C, int32_t K, int32_t pad, int32_t dil, int32_t L, float slope, float divide,
                                  void* stream) {
    if (!g || !wt_packed || !dx || dx == g || dx == residual || dx == sum_in)
        return fail(DSD_ERR_INVALID, "dsv_hgt_conv_dgrad: null argument / in-place call");
    DSD_TRY(voc_check_shape("dsv_hgt_conv_dgrad", B, L));
    if (!hgt_ch_ok(Cg) || !hgt_ch_ok(C) || !hgt_reach_ok(K, dil, pad) || divide == 0.f)
        return fail(DSD_ERR_INVALID, "dsv_hgt_conv_dgrad: bad shape (Cg=%d C=%d in [1, 1024], K=%d pad=%d dil=%d divide=%g); taps must stay within +-%d samples",
                    Cg, C, K, pad, dil, (double)divide, kVocHaloWide);
    HgtDgradParams p{};
    p.g = g; p.wp = reinterpret_cast<const float4*>(wt_packed); p.xs = x_saved; p.res = residual; p.sum_in = sum_in; p.dx = dx;
    p.Cg = Cg; p.rows = C; p.KT = K; p.pad = (K - 1) * dil - pad; p.dil = dil; p.L = L; p.LS = voc_ls(L); p.slope = slope; p.divide = divide;
    const bool wide = pad > kVocHalo || p.pad > kVocHalo;
    hipStream_t st = (hipStream_t)stream;
    if (C <= 32) { if (wide) hgt_dgrad_launch<4, 4, kVocHaloWide>(p, B, st); else hgt_dgrad_launch<4, 4, kVocHalo>(p, B, st); }
    else { if (wide) hgt_dgrad_launch<2, 2, kVocHaloWide>(p, B, st); else hgt_dgrad_launch<2, 2, kVocHalo>(p, B, st); }
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgt_conv_wgrad(const float* g, const float* x, float* workspace, int64_t workspace_floats, float* dw, int32_t B, int32_t Co,
                                  int32_t Ci, int32_t K, int32_t pad, int32_t dil, int32_t L, int32_t up, float slope, void* stream) {
    if (!g || !x || !workspace || !dw) return fail(DSD_ERR_INVALID, "dsv_hgt_conv_wgrad: null argument");
    DSD_TRY(voc_check_shape("dsv_hgt_conv_wgrad", B, L));
    const int64_t need = dsv_hgt_wgrad_workspace_floats(B, L, Co, Ci, K, up);
    if (need < 0 || !hgt_reach_ok(K, dil, pad))
        return fail(DSD_ERR_INVALID, "dsv_hgt_conv_wgrad: bad shape (Co=%d Ci=%d in [1, 1024], K=%d pad=%d dil=%d up=%d in [1, 64], L * up <= 2^30); taps "
                    "must stay within +-%d samples", Co, Ci, K, pad, dil, up, kVocHaloWide);
    if (workspace_floats < need)
        return fail(DSD_ERR_INVALID, "dsv_hgt_conv_wgrad: the workspace holds %lld floats, dsv_hgt_wgrad_workspace_floats asks for %lld",
                    (long long)workspace_floats, (long long)need);
    HgtWgradParams p{};
    p.g = g; p.x = x; p.part = workspace; p.Co = Co; p.U = up; p.rows = Co * up; p.Ci = Ci; p.K = K; p.pad = pad; p.dil = dil; p.N = K * Ci;
    p.L = L; p.LSx = voc_ls(L); p.LSg = voc_ls(L * up); p.nch = voc_splits(L, kSplitK); p.slope = slope;
    const int64_t nsplit = (int64_t)B * p.nch, n = (int64_t)p.rows * p.N;
    if (nsplit > 0x7fffffff / 2 || n > 0x7fffffff / 2 || (p.rows + 127) / 128 > 65535 || (p.N + 63) / 64 > 65535)
        return fail(DSD_ERR_INVALID, "dsv_hgt_conv_wgrad: B * splits = %lld or rows * columns = %lld is too large", (long long)nsplit, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hgt_wgrad, dim3((unsigned)nsplit, (unsigned)((p.N + 63) / 64), (unsigned)((p.rows + 127) / 128)), dim3(kThreads), 0, st, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_split_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)workspace, dw, (int)n, (int)nsplit);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsv_hgt_bias_workspace_floats(int32_t B, int32_t C, int32_t L) {
    if (!voc_shape_ok(B, L) || !hgt_ch_ok(C)) return -1;
    return 2 * (int64_t)C * B * voc_splits(L, kHgtSumChunk);                             // doubles, counted in floats
}

// partial sums per (channel, batch row, chunk) + one reduce; the workspace was checked by the caller
static int hgt_rowsum_launch(const float* g, float* workspace, float* db, int B, int C, int L, hipStream_t st) {
    const int nch = voc_splits(L, kHgtSumChunk);
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(k_hgt_rowsum_part, dim3((unsigned)nch, (unsigned)C, (unsigned)B), dim3(256), 0, st, g, part, C, L, voc_ls(L), nch);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_hgt_rowsum_reduce, dim3((unsigned)C), dim3(256), 0, st, (const double*)part, db, (int)((int64_t)B * nch));
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

static int hgt_bias_ws_check(const char* who, const float* workspace, int64_t workspace_floats, int B, int C, int L) {
    const int64_t need = dsv_hgt_bias_workspace_floats(B, C, L);
    if (need < 0 || (int64_t)B * voc_splits(L, kHgtSumChunk) > 0x7fffffff)
        return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d C=%d in [1, 1024] L=%d)", who, B, C, L);
    if (!workspace || ((uintptr_t)workspace & 7))
        return fail(DSD_ERR_INVALID, "%s: the workspace must be present and aligned to 8 bytes (float64 sums)", who);
    if (workspace_floats < need)
        return fail(DSD_ERR_INVALID, "%s: the workspace holds %lld floats, dsv_hgt_bias_workspace_floats asks for %lld", who, (long long)workspace_floats,
                    (long long)need);
    return DSD_OK;
}

extern "C" int dsv_hgt_bias_grad(const float* g, float* workspace, int64_t workspace_floats, float* db, int32_t B, int32_t C, int32_t L, void* stream) {
    if (!g || !db) return fail(DSD_ERR_INVALID, "dsv_hgt_bias_grad: null argument");
    DSD_TRY(voc_check_shape("dsv_hgt_bias_grad", B, L));
    DSD_TRY(hgt_bias_ws_check("dsv_hgt_bias_grad", workspace, workspace_floats, B, C, L));
    return hgt_rowsum_launch(g, workspace, db, B, C, L, (hipStream_t)stream);
}

extern "C" int dsv_hgt_upsample_dgrad(const float* g, const float* w, const float* x_saved, float* dx, int32_t B, int32_t Ci, int32_t Co, int32_t up,
                                      int32_t K, int32_t L_in, float slope, float divide, void* stream) {
    if (!g || !w || !x_saved || !dx || dx == g) return fail(DSD_ERR_INVALID, "dsv_hgt_upsample_dgrad: null argument / in-place call");
    DSD_TRY(voc_check_shape("dsv_hgt_upsample_dgrad", B, L_in));
    if (!hgt_ch_ok(Ci) || !hgt_ch_ok(Co) || up < 1 || up > 64 || K < up || K > 128 || ((K - up) & 1) || divide == 0.f || (int64_t)L_in * up > (1 << 30))
        return fail(DSD_ERR_INVALID, "dsv_hgt_upsample_dgrad: bad shape (Ci=%d Co=%d in [1, 1024], up=%d in [1, 64], K=%d in [up, 128] with K - up even, "
                    "L * up <= 2^30, divide=%g)", Ci, Co, up, K, (double)divide);
    const int LS_in = voc_ls(L_in), L_out = L_in * up;
    hipLaunchKernelGGL(k_hgt_up_dgrad, dim3((unsigned)((LS_in + 255) / 256), (unsigned)Ci, (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, w, x_saved, dx,
                       Ci, Co, up, K, (K - up) / 2, L_in, LS_in, L_out, voc_ls(L_out), slope, divide);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgt_tanh_backward(const float* gy, const float* y, float* out, int32_t B, int32_t L, void* stream) {
    if (!gy || !y || !out) return fail(DSD_ERR_INVALID, "dsv_hgt_tanh_backward: null argument");
    DSD_TRY(voc_check_shape("dsv_hgt_tanh_backward", B, L));
    const int LS = voc_ls(L);
    hipLaunchKernelGGL(k_hgt_tanh_bwd, dim3((unsigned)((LS + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, gy, y, out, L, LS);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgt_noise_conv_backward(const float* g, const float* har, const float* w, float* workspace, int64_t workspace_floats, float* dw,
                                           float* db, float* dhar, int32_t B, int32_t C, int32_t K, int32_t stride, int32_t pad, int32_t L_har,
                                           int32_t L_out, int32_t first, void* stream) {
    if (!g || !har || !w || !dw || !db || !dhar) return fail(DSD_ERR_INVALID, "dsv_hgt_noise_conv_backward: null argument");
    DSD_TRY(voc_check_shape("dsv_hgt_noise_conv_backward", B, L_har));
    if (!hgt_ch_ok(C) || K < 1 || K > 65535 || stride < 1 || pad < 0 || L_out < 1 || (int64_t)(L_har + 2 * (int64_t)pad - K) / stride + 1 != L_out ||
        (int64_t)L_har + 2 * (int64_t)pad < K)
        return fail(DSD_ERR_INVALID, "dsv_hgt_noise_conv_backward: bad shape (C=%d in [1, 1024], K=%d stride=%d pad=%d L_har=%d L_out=%d)", C, K, stride, pad,
                    L_har, L_out);
    DSD_TRY(hgt_bias_ws_check("dsv_hgt_noise_conv_backward", workspace, workspace_floats, B, C, L_out));
    const int LSh = voc_ls(L_har), LSo = voc_ls(L_out);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hgt_noise_wgrad, dim3((unsigned)K, (unsigned)C), dim3(256), 0, st, g, har, dw, B, C, K, stride, pad, L_har, LSh, L_out, LSo);
    HIP_TRY(hipGetLastError());
    DSD_TRY(hgt_rowsum_launch(g, workspace, db, B, C, L_out, st));
    hipLaunchKernelGGL(k_hgt_noise_dhar, dim3((unsigned)((LSh + 255) / 256), (unsigned)B), dim3(256), 0, st, g, w, dhar, C, K, stride, pad, L_har, LSh, L_out,
                       LSo, first ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgt_source_mix(const float* f0, const float* sines_ws, const float* noise, float* sines, int32_t B, int32_t T, int32_t up, int32_t H,
                                  float sine_amp, float noise_std, float voiced_threshold, void* stream) {
    if (!f0 || !sines_ws || !noise || !sines) return fail(DSD_ERR_INVALID, "dsv_hgt_source_mix: null argument");
    if (B < 1 || B > 65535 || T < 1 || up < 1 || H < 1 || H > 64 || (int64_t)T * up > (1 << 30))
        return fail(DSD_ERR_INVALID, "dsv_hgt_source_mix: bad shape (B=%d T=%d up=%d H=%d)", B, T, up, H);
    HgtMixParams p{};
    p.f0 = f0; p.sw = sines_ws; p.noise = noise; p.sines = sines; p.T = T; p.up = up; p.L = T * up; p.H = H;
    p.noise_std = noise_std; p.sine_amp = sine_amp; p.voiced_threshold = voiced_threshold;
    hipLaunchKernelGGL(k_hgt_source_mix, dim3((unsigned)((p.L + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgt_source_backward(const float* dhar, const float* har, const float* sines, float* dw, float* db, int32_t B, int32_t L, int32_t H,
                                       void* stream) {
    if (!dhar || !har || !sines || !dw || !db) return fail(DSD_ERR_INVALID, "dsv_hgt_source_backward: null argument");
    DSD_TRY(voc_check_shape("dsv_hgt_source_backward", B, L));
    if (H < 1 || H > 64) return fail(DSD_ERR_INVALID, "dsv_hgt_source_backward: H=%d must be in [1, 64]", H);
    hipLaunchKernelGGL(k_hgt_source_bwd, dim3((unsigned)(H + 1)), dim3(256), 0, (hipStream_t)stream, dhar, har, sines, dw, db, B, L, voc_ls(L), H);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
