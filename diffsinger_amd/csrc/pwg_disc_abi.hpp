// pwg_disc_abi.hpp - host side of the ParallelWaveGAN discriminator (C ABI in include/dsv.h, section "PWG discriminator"; kernels in
// pwg_disc.hpp); included at the end of dsd.hip behind voc_stft_loss_abi.hpp.  Every entry point validates on the host and refuses with
// DSD_ERR_INVALID before any launch; nothing allocates or synchronises.
#include "pwg_disc.hpp"
#include "voc_train_host.hpp"

extern "C" int32_t dsv_pwgd_tile(void) { return kPwgdTile; }
extern "C" int32_t dsv_pwgd_wgrad_split(void) { return kPwgdSplit; }

extern "C" int64_t dsv_pwgd_wgrad_workspace_floats(int32_t B, int32_t T) {
    if (!voc_shape_ok(B, T)) return -1;
    return (int64_t)B * voc_splits(T, kPwgdSplit) * kPwgdWgFloats;
}

extern "C" int64_t dsv_pwgd_edge_workspace_floats(int32_t B, int32_t T) {
    if (!voc_shape_ok(B, T)) return -1;
    return (int64_t)B * voc_splits(T, kPwgdEdgeSplit) * kPwgdC * 4;
}

static int pwgd_check_slope(const char* who, float slope) {
    if (!(slope > 0.f && slope < 1.f)) return fail(DSD_ERR_INVALID, "%s: negative_slope=%g must be in (0, 1)", who, (double)slope);
    return DSD_OK;
}
static int pwgd_check_grid(const char* who, int64_t blocks) {
    if (blocks > 65535) return fail(DSD_ERR_INVALID, "%s: B * splits = %lld exceeds 65535 workgroups", who, (long long)blocks);
    return DSD_OK;
}

extern "C" int dsv_pwgd_layer(const float* in, const float* w_packed, const float* bias, const float* saved, float* out, int32_t B, int32_t T,
                              int32_t dil, float slope, int32_t backward, void* stream) {
    if (!in || !w_packed || !out) return fail(DSD_ERR_INVALID, "dsv_pwgd_layer: null argument");
    if (in == out) return fail(DSD_ERR_INVALID, "dsv_pwgd_layer: out must not alias in");
    DSD_TRY(voc_check_shape("dsv_pwgd_layer", B, T, 'T'));
    DSD_TRY(pwgd_check_slope("dsv_pwgd_layer", slope));
    if (dil < 1 || dil > kPwgdHalo) return fail(DSD_ERR_INVALID, "dsv_pwgd_layer: dil=%d must be in [1, %d]", dil, kPwgdHalo);
    if (backward && bias) return fail(DSD_ERR_INVALID, "dsv_pwgd_layer: the data gradient takes no bias");
    if (!backward && saved) return fail(DSD_ERR_INVALID, "dsv_pwgd_layer: the forward takes no saved activation");
    PwgdLayerParams p{};
    p.in = in; p.wp = reinterpret_cast<const float4*>(w_packed); p.bias = bias; p.saved = saved; p.out = out;
    p.T = T; p.LS = voc_ls(T); p.dil = dil; p.slope = slope;
    const dim3 grid((unsigned)((p.LS + kPwgdTile - 1) / kPwgdTile), (unsigned)B);
    if (backward) hipLaunchKernelGGL((k_pwgd_layer<true>), grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((k_pwgd_layer<false>), grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgd_wgrad(const float* g, const float* a_prev, float* workspace, float* dw, float* db, int32_t B, int32_t T, int32_t dil,
                              void* stream) {
    if (!g || !a_prev || !workspace || !dw) return fail(DSD_ERR_INVALID, "dsv_pwgd_wgrad: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgd_wgrad", B, T, 'T'));
    if (dil < 1 || dil > kPwgdHalo) return fail(DSD_ERR_INVALID, "dsv_pwgd_wgrad: dil=%d must be in [1, %d]", dil, kPwgdHalo);
    PwgdWgradParams p{};
    p.g = g; p.a = a_prev; p.part = workspace; p.T = T; p.LS = voc_ls(T); p.dil = dil; p.nch = voc_splits(T, kPwgdSplit);
    const int64_t nsplit = (int64_t)B * p.nch;
    if (nsplit > 0x7fffffff) return fail(DSD_ERR_INVALID, "dsv_pwgd_wgrad: B * splits = %lld is too large", (long long)nsplit);
    hipLaunchKernelGGL(k_pwgd_wgrad, dim3((unsigned)nsplit), dim3(kThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pwgd_wgrad_reduce, dim3(kPwgdWgFloats / 64), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, db,
                       (int)nsplit);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgd_first(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t T, float slope, void* stream) {
    if (!x || !w || !out) return fail(DSD_ERR_INVALID, "dsv_pwgd_first: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgd_first", B, T, 'T'));
    DSD_TRY(pwgd_check_slope("dsv_pwgd_first", slope));
    const int LS = voc_ls(T);
    hipLaunchKernelGGL(k_pwgd_first, dim3((unsigned)((LS + 255) / 256), kPwgdC, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, w, bias, out, T, LS,
                       slope);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgd_first_backward(const float* g0, const float* x, const float* w, float* workspace, float* dw, float* db, float* dx, int32_t B,
                                       int32_t T, void* stream) {
    if (!g0 || !x || !w || !workspace || !dw) return fail(DSD_ERR_INVALID, "dsv_pwgd_first_backward: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgd_first_backward", B, T, 'T'));
    const int LS = voc_ls(T), nch = voc_splits(T, kPwgdEdgeSplit);
    DSD_TRY(pwgd_check_grid("dsv_pwgd_first_backward", (int64_t)B * nch));
    hipLaunchKernelGGL(k_pwgd_edge_wgrad, dim3(kPwgdC, (unsigned)(B * nch)), dim3(256), 0, (hipStream_t)stream, g0, x, workspace, T,
                       (size_t)kPwgdC * LS, (size_t)LS, (size_t)LS, (size_t)0, nch);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pwgd_edge_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, db, B * nch, 1);
    HIP_TRY(hipGetLastError());
    if (dx) {
        hipLaunchKernelGGL(k_pwgd_first_dx, dim3((unsigned)((LS + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g0, w, dx, T, LS);
        HIP_TRY(hipGetLastError());
    }
    return DSD_OK;
}

extern "C" int dsv_pwgd_last(const float* a, const float* w, const float* bias, float* out, int32_t B, int32_t T, void* stream) {
    if (!a || !w || !out) return fail(DSD_ERR_INVALID, "dsv_pwgd_last: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgd_last", B, T, 'T'));
    const int LS = voc_ls(T);
    hipLaunchKernelGGL(k_pwgd_last, dim3((unsigned)((LS + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a, w, bias, out, T, LS);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgd_last_backward(const float* gp, const float* a, const float* w, float* workspace, float* dw, float* db, float* ga, int32_t B,
                                      int32_t T, float slope, void* stream) {
    if (!gp || !a || !w || !workspace || !dw || !ga) return fail(DSD_ERR_INVALID, "dsv_pwgd_last_backward: null argument");
    DSD_TRY(voc_check_shape("dsv_pwgd_last_backward", B, T, 'T'));
    DSD_TRY(pwgd_check_slope("dsv_pwgd_last_backward", slope));
    const int LS = voc_ls(T), nch = voc_splits(T, kPwgdEdgeSplit);
    DSD_TRY(pwgd_check_grid("dsv_pwgd_last_backward", (int64_t)B * nch));
    hipLaunchKernelGGL(k_pwgd_edge_wgrad, dim3(kPwgdC, (unsigned)(B * nch)), dim3(256), 0, (hipStream_t)stream, gp, a, workspace, T, (size_t)LS,
                       (size_t)0, (size_t)kPwgdC * LS, (size_t)LS, nch);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pwgd_edge_reduce, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, db, B * nch, 0);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pwgd_last_dgrad, dim3((unsigned)((LS + 255) / 256), kPwgdC, (unsigned)B), dim3(256), 0, (hipStream_t)stream, gp, a, w, ga, T,
                       LS, slope);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

static int pwgd_loss_blocks(int64_t n) {
    const int64_t want = (n + 4 * kPwgdLossThreads - 1) / (4 * kPwgdLossThreads);
    return (int)(want < 1 ? 1 : want > kPwgdLossMaxBlocks ? kPwgdLossMaxBlocks : want);
}

extern "C" int64_t dsv_pwgd_lsgan_workspace_floats(int64_t n) {
    if (n < 1 || n > ((int64_t)1 << 40)) return -1;
    return 2 * (int64_t)pwgd_loss_blocks(n);                                                // doubles, counted in floats
}

static int pwgd_loss_check(const char* who, const void* a, const void* b, const void* c, int64_t n) {
    if (!a || !b || !c) return fail(DSD_ERR_INVALID, "%s: null argument", who);
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(DSD_ERR_INVALID, "%s: bad shape (n=%lld must be in [1, 2^40])", who, (long long)n);
    return DSD_OK;
}

extern "C" int dsv_pwgd_lsgan(const float* d, float target, float* workspace, float* out, int64_t n, void* stream) {
    DSD_TRY(pwgd_loss_check("dsv_pwgd_lsgan", d, workspace, out, n));
    DSD_TRY(voc_check_f64_workspace("dsv_pwgd_lsgan", workspace, "it holds float64 sums"));
    const int nb = pwgd_loss_blocks(n);
    double* ws = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(k_pwgd_lsgan_partial, dim3((unsigned)nb), dim3(kPwgdLossThreads), 0, (hipStream_t)stream, d, target, ws, (long long)n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pwgd_lsgan_final, dim3(1), dim3(kPwgdLossThreads), 0, (hipStream_t)stream, (const double*)ws, out, nb, (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_pwgd_lsgan_backward(const float* d, float target, const float* grad_out, float* G, int64_t n, void* stream) {
    DSD_TRY(pwgd_loss_check("dsv_pwgd_lsgan_backward", d, grad_out, G, n));
    const int64_t want = (n + kPwgdLossThreads - 1) / kPwgdLossThreads;
    const unsigned nb = (unsigned)(want > 16384 ? 16384 : want);
    hipLaunchKernelGGL(k_pwgd_lsgan_backward, dim3(nb), dim3(kPwgdLossThreads), 0, (hipStream_t)stream, d, target, grad_out, G, (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
