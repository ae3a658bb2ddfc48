// pwg_train_abi.hpp - host side of ParallelWaveGAN generator training (C ABI in include/dsv.h, section "PWG generator training"; kernels in
// pwg_train.hpp); included at the end of dsd.hip behind pwg_disc_abi.hpp.  Every entry point validates on the host and refuses with
// DSD_ERR_INVALID before any launch; nothing allocates or synchronises.
#include "pwg_train.hpp"
#include "voc_train_host.hpp"

extern "C" int32_t dsv_pwgt_wgrad_split(void) { return kSplitK; }

static bool pwgt_aux_ok(int naux) { return naux >= 0 && naux <= kPwgMaxAux && (naux % 8) == 0; }

static int pwgt_check_aux(const char* who, int naux, const void* c) {
    if (!pwgt_aux_ok(naux) || (naux && !c))
        return fail(DSD_ERR_INVALID, "%s: aux=%d must be a multiple of 8 in [0, %d] with its tensor present", who, naux, kPwgMaxAux);
    return DSD_OK;
}

extern "C" int64_t dsv_pwgt_wgrad_workspace_floats(int32_t B, int32_t L, int32_t n_cols) {
    if (!voc_shape_ok(B, L) || n_cols < 8 || n_cols > 3 * kPwgRes + kPwgMaxAux || (n_cols % 8)) return -1;
    return (int64_t)B * voc_splits(L, kSplitK) * ((int64_t)kPwgGate * n_cols + kPwgGate);
}

extern "C" int64_t dsv_pwgt_upsample_workspace_floats(int64_t rows, int32_t scale) {
    if (rows < 1 || rows > 65535 || scale < 1 || scale > 64) return -1;
    return 2 * rows * (2 * scale + 1);                                                      // doubles, counted in floats
}

extern "C" int dsv_pwgt_layer(const float* x, const float* c, const float* w1_packed, const float* b1, const float* w2_packed, const float* b2,
                              float* x_out, float* skip, float* a_out, int32_t B, int32_t L, int32_t n_aux, int32_t dil, int32_t first,
                              void* stream) {
    if (!x || !w1_packed || !w2_packed || !x_out || !skip || !a_out || x == x_out)
        return fail(DSD_ERR_INVALID, "dsv_pwgt_layer: null argument / in-place call");
    DSD_TRY(voc_check_shape("dsv_pwgt_layer", B, L));
    DSD_TRY(pwgt_check_aux("dsv_pwgt_layer", n_aux, c));
    if (dil < 1) return fail(DSD_ERR_INVALID, "dsv_pwgt_layer: dil=%d must be positive", dil);
    if (first_on_device(41)) HIP_TRY(hipFuncSetAttribute((const void*)k_pwgt_layer, hipFuncAttributeMaxDynamicSharedMemorySize, kPwgLayerLdsBytes));
    PwgtLayerParams q{};
    PwgLayerParams& p = q.f;
    p.x = x; p.c = n_aux ? c : nullptr; p.w1p = reinterpret_cast<const float4*>(w1_packed); p.b1 = b1;
    p.w2p = reinterpret_cast<const float4*>(w2_packed); p.b2 = b2; p.x_out = x_out; p.skip = skip;
    p.L = L; p.LS = voc_ls(L); p.dil = dil; p.naux = n_aux; p.first = first ? 1 : 0;
    q.a_out = a_out;
    hipLaunchKernelGGL(k_pwgt_layer, dim3((unsigned)(p.LS / 32), (unsigned)B), dim3(kThreads), kPwgLayerLdsBytes, (hipStream_t)stream, q);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgt_gate_backward(const float* dx_next, const float* d_skip, const float* a, const float* w2t_packed, float* da, int32_t B,
                                      int32_t L, void* stream) {
    if (!d_skip || !a || !w2t_packed || !da) return fail(DSD_ERR_INVALID, "dsv_pwgt_gate_backward: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_gate_backward", B, L));
    PwgtGateBwdParams p{};
    p.dxp = dx_next; p.ds = d_skip; p.a = a; p.w2tp = reinterpret_cast<const float4*>(w2t_packed); p.da = da; p.L = L; p.LS = voc_ls(L);
    hipLaunchKernelGGL(k_pwgt_gate_bwd, dim3((unsigned)(p.LS / 32), (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgt_conv_backward(const float* da, const float* dx_next, const float* w1t_packed, const float* wauxt_packed, float* dx, float* dc,
                                      int32_t B, int32_t L, int32_t n_aux, int32_t dil, int32_t first, void* stream) {
    if (!da || !w1t_packed || !dx || dx == dx_next) return fail(DSD_ERR_INVALID, "dsv_pwgt_conv_backward: null argument / in-place call");
    DSD_TRY(voc_check_shape("dsv_pwgt_conv_backward", B, L));
    if (!pwgt_aux_ok(n_aux) || (n_aux && (!dc || !wauxt_packed)))
        return fail(DSD_ERR_INVALID, "dsv_pwgt_conv_backward: aux=%d must be a multiple of 8 in [0, %d] with dc and its matrix present", n_aux, kPwgMaxAux);
    if (dil < 1) return fail(DSD_ERR_INVALID, "dsv_pwgt_conv_backward: dil=%d must be positive", dil);
    PwgtConvBwdParams p{};
    p.da = da; p.dxp = dx_next; p.w1tp = reinterpret_cast<const float4*>(w1t_packed);
    p.wauxtp = n_aux ? reinterpret_cast<const float4*>(wauxt_packed) : nullptr; p.dx = dx; p.dc = n_aux ? dc : nullptr;
    p.L = L; p.LS = voc_ls(L); p.dil = dil; p.naux = n_aux; p.first = first ? 1 : 0;
    hipLaunchKernelGGL(k_pwgt_conv_bwd, dim3((unsigned)(p.LS / 32), (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

// partials + reduction of one 128-row gradient; out = [128][N] then [128]
static int pwgt_wgrad_launch(const char* who, PwgtWgradParams& p, float* workspace, float* out, int B, hipStream_t s) {
    p.part = workspace; p.nch = voc_splits(p.L, kSplitK);
    const int64_t nsplit = (int64_t)B * p.nch;
    if (nsplit > 0x7fffffff / 2) return fail(DSD_ERR_INVALID, "%s: B * splits = %lld is too large", who, (long long)nsplit);
    const int n = kPwgGate * p.N + kPwgGate;
    hipLaunchKernelGGL(k_pwgt_wgrad, dim3((unsigned)nsplit, (unsigned)((p.N + 63) / 64)), dim3(kThreads), 0, s, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_split_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)workspace, out, n, (int)nsplit);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgt_wgrad_conv(const float* da, const float* x, const float* c, float* workspace, float* out, int32_t B, int32_t L, int32_t n_aux,
                                   int32_t dil, void* stream) {
    if (!da || !x || !workspace || !out) return fail(DSD_ERR_INVALID, "dsv_pwgt_wgrad_conv: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_wgrad_conv", B, L));
    DSD_TRY(pwgt_check_aux("dsv_pwgt_wgrad_conv", n_aux, c));
    if (dil < 1) return fail(DSD_ERR_INVALID, "dsv_pwgt_wgrad_conv: dil=%d must be positive", dil);
    PwgtWgradParams p{};
    p.LS = voc_ls(L); p.L = L;
    p.p0 = da; p.p1 = da + (size_t)kPwgRes * p.LS; p.bs0 = p.bs1 = (size_t)kPwgGate * p.LS; p.scale0 = 1.f;
    p.x = x; p.c = n_aux ? c : nullptr; p.dil = dil; p.naux = n_aux; p.N = 3 * kPwgRes + n_aux; p.qmode = 0;
    return pwgt_wgrad_launch("dsv_pwgt_wgrad_conv", p, workspace, out, B, (hipStream_t)stream);
}

extern "C" int dsv_pwgt_wgrad_out(const float* dx_next, const float* d_skip, const float* a, float* workspace, float* out, int32_t B, int32_t L,
                                  void* stream) {
    if (!d_skip || !a || !workspace || !out) return fail(DSD_ERR_INVALID, "dsv_pwgt_wgrad_out: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_wgrad_out", B, L));
    PwgtWgradParams p{};
    p.LS = voc_ls(L); p.L = L;
    // P rows follow the forward's second matrix: 0..63 conv1x1_out (s dx'), 64..127 conv1x1_skip (dS).  Without dx' (the last block) the out rows
    // of the result are zeros and the caller drops them.
    p.p0 = dx_next; p.p1 = d_skip; p.bs0 = p.bs1 = (size_t)kPwgRes * p.LS; p.scale0 = sqrtf(0.5f);
    p.a = a; p.dil = 1; p.naux = 0; p.N = kPwgRes; p.qmode = 1;
    return pwgt_wgrad_launch("dsv_pwgt_wgrad_out", p, workspace, out, B, (hipStream_t)stream);
}

extern "C" int dsv_pwgt_wgrad_relu(const float* g, const float* saved, float* workspace, float* out, int32_t B, int32_t L, void* stream) {
    if (!g || !saved || !workspace || !out) return fail(DSD_ERR_INVALID, "dsv_pwgt_wgrad_relu: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_wgrad_relu", B, L));
    PwgtWgradParams p{};
    p.LS = voc_ls(L); p.L = L;
    p.p0 = g; p.p1 = nullptr; p.bs0 = p.bs1 = (size_t)kPwgRes * p.LS; p.scale0 = 1.f;
    p.x = saved; p.dil = 1; p.naux = 0; p.N = kPwgRes; p.qmode = 2;
    return pwgt_wgrad_launch("dsv_pwgt_wgrad_relu", p, workspace, out, B, (hipStream_t)stream);
}

extern "C" int dsv_pwgt_rowdot(const float* P, const float* Q, float* out, int32_t B, int32_t C, int32_t L, int32_t p_per_channel,
                               int32_t q_per_channel, int32_t relu_q, void* stream) {
    if (!P || !Q || !out) return fail(DSD_ERR_INVALID, "dsv_pwgt_rowdot: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_rowdot", B, L));
    if (C < 1 || C > 65535) return fail(DSD_ERR_INVALID, "dsv_pwgt_rowdot: C=%d must be in [1, 65535]", C);
    const size_t LS = (size_t)voc_ls(L);
    hipLaunchKernelGGL(k_pwgt_rowdot, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, P, Q, out, B, L, p_per_channel ? (size_t)C * LS : LS,
                       p_per_channel ? LS : (size_t)0, q_per_channel ? (size_t)C * LS : LS, q_per_channel ? LS : (size_t)0, relu_q ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgt_last_dgrad(const float* g, const float* saved, const float* w, float* out, int32_t B, int32_t C, int32_t L, void* stream) {
    if (!g || !saved || !w || !out) return fail(DSD_ERR_INVALID, "dsv_pwgt_last_dgrad: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_last_dgrad", B, L));
    if (C < 1 || C > 65535) return fail(DSD_ERR_INVALID, "dsv_pwgt_last_dgrad: C=%d must be in [1, 65535]", C);
    const int LS = voc_ls(L);
    hipLaunchKernelGGL(k_pwgt_last_dgrad, dim3((unsigned)((LS + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0, (hipStream_t)stream, g, saved, w,
                       out, C, L, LS);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgt_relu_mask(const float* g, const float* saved, float* out, float scale, int64_t rows, int32_t L, void* stream) {
    if (!g || !saved || !out) return fail(DSD_ERR_INVALID, "dsv_pwgt_relu_mask: null argument");
    if (rows < 1 || rows > 65535 || L < 1 || L > (1 << 30)) return fail(DSD_ERR_INVALID, "dsv_pwgt_relu_mask: bad shape (rows=%lld L=%d)", (long long)rows, L);
    const int LS = voc_ls(L);
    hipLaunchKernelGGL(k_pwgt_relu_mask, dim3((unsigned)((LS + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, g, saved, out, scale, L,
                       LS);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgt_upsample_backward(const float* g, const float* in, const float* filter, float* workspace, float* din, float* dw, int64_t rows,
                                          int32_t L_in, int32_t scale, void* stream) {
    if (!g || !in || !filter || !workspace || !dw) return fail(DSD_ERR_INVALID, "dsv_pwgt_upsample_backward: null argument");
    if (rows < 1 || rows > 65535 || L_in < 1 || scale < 1 || scale > 64 || (int64_t)L_in * scale > (1 << 30))
        return fail(DSD_ERR_INVALID, "dsv_pwgt_upsample_backward: bad shape (rows=%lld L=%d scale=%d)", (long long)rows, L_in, scale);
    DSD_TRY(voc_check_f64_workspace("dsv_pwgt_upsample_backward", workspace));
    const int LS_in = voc_ls(L_in), LS_out = voc_ls(L_in * scale), ntap = 2 * scale + 1;
    double* ws = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(k_pwgt_up_wgrad, dim3((unsigned)ntap, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, g, in, ws, L_in, LS_in, scale, LS_out);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pwgt_up_wreduce, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, dw, (int)rows, ntap);
    HIP_TRY(hipGetLastError());
    if (din) {
        hipLaunchKernelGGL(k_pwgt_up_dgrad, dim3((unsigned)((LS_in + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, g, filter, din, L_in,
                           LS_in, scale, LS_out);
        HIP_TRY(hipGetLastError());
    }
    return DSD_OK;
}

extern "C" int dsv_pwgt_convin_wgrad(const float* g, const float* c, float* dw, int32_t B, int32_t C, int32_t K, int32_t L_out, void* stream) {
    if (!g || !c || !dw) return fail(DSD_ERR_INVALID, "dsv_pwgt_convin_wgrad: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgt_convin_wgrad", B, L_out));
    if (C < 1 || C > kPwgMaxAux || K < 1 || K > 65) return fail(DSD_ERR_INVALID, "dsv_pwgt_convin_wgrad: bad shape (C=%d in [1, %d], K=%d in [1, 65])", C, kPwgMaxAux, K);
    const int n = C * C * K;
    hipLaunchKernelGGL(k_pwgt_convin_wgrad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, c, dw, B, C, K, L_out, voc_ls(L_out),
                       voc_ls(L_out + K - 1));
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
