// voc_stft_loss_abi.hpp - host side of the STFT loss (C ABI in include/dsv.h, section "STFT loss"; kernels in voc_stft_loss.hpp); included at
// the end of dsd.hip behind voc_stft_abi.hpp (shares stft_nfft_ok, stft_fill, stft_plan, stft_zsplit).  Every entry point
// validates on the host and refuses with DSD_ERR_INVALID before any launch; nothing allocates or synchronises.
#include "voc_stft_loss.hpp"
#include "voc_train_host.hpp"

// site id of first_on_device in this file: 703.  It sets the dynamic-LDS attribute of k_stft<2, 2> - the SAME function object site 702 (dsv_istft,
// voc_stft_abi.hpp) sets: both stay, because either entry point can be the first caller of the kernel on a device.

extern "C" int dsv_stft_make_adjoint_basis(int32_t n_fft, int32_t win_length, float* adj, void* stream) {
    if (!stft_nfft_ok(n_fft)) return fail(DSD_ERR_INVALID, "dsv_stft_make_adjoint_basis: n_fft=%d is not one of 256, 512, 1024, 2048", n_fft);
    if (win_length < 1 || win_length > n_fft)
        return fail(DSD_ERR_INVALID, "dsv_stft_make_adjoint_basis: win_length=%d must be in [1, n_fft=%d]", win_length, n_fft);
    if (!adj) return fail(DSD_ERR_INVALID, "dsv_stft_make_adjoint_basis: null argument");
    hipLaunchKernelGGL(k_stft_make_adj_basis, dim3(2048), dim3(256), 0, (hipStream_t)stream, adj, n_fft, win_length);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsv_stft_adjoint_workspace_floats(int32_t B, int64_t n_frames, int32_t n_fft) {
    return dsv_istft_workspace_floats(B, n_frames, n_fft);
}

extern "C" int dsv_stft_adjoint(const float* grad_spec, const float* adj_basis, float* workspace, float* grad_wav, int32_t B, int32_t L, int32_t n_fft,
                                int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode, void* stream) {
    // the geometry is the forward's: the same checks, on the same arguments
    StftParams fwd;
    DSD_TRY(stft_fill(fwd, "dsv_stft_adjoint", grad_spec, nullptr, adj_basis, B, L, n_fft, hop, pad_l, pad_r, pad_mode));
    if (!workspace || !grad_wav) return fail(DSD_ERR_INVALID, "dsv_stft_adjoint: null argument");
    const int nF = fwd.nF;
    StftParams p{};
    p.in = grad_spec; p.basis = reinterpret_cast<const float4*>(adj_basis); p.out = workspace;
    p.N = n_fft; p.hop = n_fft; p.nF = nF;
    size_t lds;
    stft_plan(n_fft, n_fft, p.KC, p.RL, lds);
    if (first_on_device(703)) HIP_TRY(hipFuncSetAttribute((const void*)k_stft<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStftLdsBudget));
    const unsigned gx = (unsigned)((nF + kStftNF - 1) / kStftNF);
    hipLaunchKernelGGL((k_stft<2, 2>), dim3(gx, (unsigned)B, stft_zsplit(gx, (unsigned)B, n_fft, 2)), dim3(kStftThreads), lds, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    StftAdjFoldParams q{};
    q.frames = workspace; q.out = grad_wav;
    q.nF = nF; q.N = n_fft; q.hop = hop; q.pad_l = pad_l; q.pad_r = pad_r; q.reflect = pad_mode == DSV_STFT_PAD_REFLECT; q.L = L;
    hipLaunchKernelGGL(k_stft_adj_fold, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, q);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

static int stft_loss_blocks(int64_t n) {
    const int64_t want = (n + 4 * kStftLossThreads - 1) / (4 * kStftLossThreads);          // four elements per thread before the grid strides
    return (int)(want < 1 ? 1 : want > kStftLossMaxBlocks ? kStftLossMaxBlocks : want);
}

extern "C" int64_t dsv_spectral_loss_workspace_floats(int64_t n) {
    if (n < 1 || n > ((int64_t)1 << 40)) return -1;
    return 2 * (int64_t)(kStftLossHead + 3 * stft_loss_blocks(n));                          // doubles, counted in floats
}

static int stft_loss_check(const char* who, const void* a, const void* b, const void* c, const void* d, int64_t n) {
    if (!a || !b || !c || !d) return fail(DSD_ERR_INVALID, "%s: null argument", who);
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(DSD_ERR_INVALID, "%s: bad shape (n=%lld complex elements must be in [1, 2^40])", who, (long long)n);
    return voc_check_f64_workspace(who, c, "it holds float64 sums");
}

extern "C" int dsv_spectral_loss(const float* X, const float* Y, float* workspace, float* out, int64_t n, void* stream) {
    DSD_TRY(stft_loss_check("dsv_spectral_loss", X, Y, workspace, out, n));
    const int nb = stft_loss_blocks(n);
    double* ws = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(k_stft_loss_partial, dim3((unsigned)nb), dim3(kStftLossThreads), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(X),
                       reinterpret_cast<const float2*>(Y), ws, (long long)n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_stft_loss_final, dim3(1), dim3(kStftLossThreads), 0, (hipStream_t)stream, ws, out, nb, (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_spectral_loss_backward(const float* X, const float* Y, const float* workspace, const float* grad_out, float* G, int64_t n,
                                          void* stream) {
    DSD_TRY(stft_loss_check("dsv_spectral_loss_backward", X, Y, workspace, grad_out, n));
    if (!G) return fail(DSD_ERR_INVALID, "dsv_spectral_loss_backward: null argument");
    const int64_t want = (n + kStftLossThreads - 1) / kStftLossThreads;
    const unsigned nb = (unsigned)(want > 16384 ? 16384 : want);
    hipLaunchKernelGGL(k_stft_loss_backward, dim3(nb), dim3(kStftLossThreads), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(X),
                       reinterpret_cast<const float2*>(Y), reinterpret_cast<const double*>(workspace), grad_out, reinterpret_cast<float2*>(G),
                       (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
