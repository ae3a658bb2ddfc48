// voc_stft_abi.hpp - host side of the STFT family (C ABI in include/dsv.h, section "STFT"; kernels in voc_stft.hpp); included at the end of
// dsd.hip (one translation unit: shares fail(), HIP_TRY, first_on_device).  Every entry point validates on the host and refuses with
// DSD_ERR_INVALID before any launch; nothing allocates or synchronises.
#include "voc_stft.hpp"

#include "../../include/dsv.h"

// site ids of first_on_device in this file: 700 .. 702
static bool stft_nfft_ok(int n_fft) { return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048; }

// The chunk of the contraction (KC samples, a power of two) and the LDS row length RL = min(hop, KC): the largest chunk whose staged window
// of 64 frames fits the budget (voc_stft.hpp).
static void stft_plan(int n_fft, int hop, int& KC, int& RL, size_t& lds_bytes) {
    for (KC = n_fft; KC >= 8; KC >>= 1) {
        RL = hop < KC ? hop : KC;
        const size_t rows = (size_t)kStftNF - 1 + (size_t)((KC + RL - 1) / RL);
        lds_bytes = rows * (size_t)(RL + 2) * sizeof(float);
        if (lds_bytes <= (size_t)kStftLdsBudget) return;
    }
    KC = 8; RL = hop < 8 ? hop : 8;
    lds_bytes = ((size_t)kStftNF - 1 + (size_t)((KC + RL - 1) / RL)) * (size_t)(RL + 2) * sizeof(float);
}

extern "C" int64_t dsv_stft_basis_floats(int32_t n_fft, int32_t which) {
    if (!stft_nfft_ok(n_fft) || which < 0 || which > DSV_STFT_BASIS_ADJ)
        return fail(DSD_ERR_INVALID, "dsv_stft_basis_floats: n_fft=%d is not one of 256, 512, 1024, 2048, or which=%d is not a basis (0 forward, 1 inverse, 2 adjoint)", n_fft, which);
    return (int64_t)n_fft * n_fft + (which == DSV_STFT_BASIS_INV ? n_fft : 0);
}

extern "C" int dsv_stft_make_basis(int32_t n_fft, int32_t win_length, float* fwd, float* inv, void* stream) {
    if (!stft_nfft_ok(n_fft)) return fail(DSD_ERR_INVALID, "dsv_stft_make_basis: n_fft=%d is not one of 256, 512, 1024, 2048", n_fft);
    if (win_length < 1 || win_length > n_fft) return fail(DSD_ERR_INVALID, "dsv_stft_make_basis: win_length=%d must be in [1, n_fft=%d]", win_length, n_fft);
    if (!fwd && !inv) return fail(DSD_ERR_INVALID, "dsv_stft_make_basis: no output asked for (fwd, inv)");
    hipLaunchKernelGGL(k_stft_make_basis, dim3(2048), dim3(256), 0, (hipStream_t)stream, fwd, inv, n_fft, win_length);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsv_stft_frames(int64_t L, int32_t n_fft, int32_t hop, int32_t pad_l, int32_t pad_r) {
    if (L < 1 || n_fft < 1 || hop < 1 || pad_l < 0 || pad_r < 0 || L + pad_l + pad_r < n_fft) return -1;
    return 1 + (L + pad_l + pad_r - n_fft) / hop;
}

extern "C" int64_t dsv_istft_samples(int64_t n_frames, int32_t n_fft, int32_t hop, int32_t center) {
    if (n_frames < 1 || n_fft < 1 || hop < 1) return -1;
    const int64_t n = n_fft + (int64_t)hop * (n_frames - 1) - (center ? 2 * (int64_t)(n_fft / 2) : 0);
    return n < 0 ? 0 : n;
}

static int stft_fill(StftParams& p, const char* who, const float* wav, const int32_t* lengths, const float* basis, int32_t B, int32_t L, int32_t n_fft,
                     int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode) {
    if (!wav || !basis) return fail(DSD_ERR_INVALID, "%s: null argument", who);
    if (!stft_nfft_ok(n_fft)) return fail(DSD_ERR_INVALID, "%s: n_fft=%d is not one of 256, 512, 1024, 2048", who, n_fft);
    if (hop < 1 || hop > n_fft) return fail(DSD_ERR_INVALID, "%s: hop=%d must be in [1, n_fft=%d]", who, hop, n_fft);
    if (B < 1 || B > 65535 || L < 1 || L > (1 << 30)) return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d in [1, 65535], L=%d in [1, 2^30])", who, B, L);
    if (pad_mode != DSV_STFT_PAD_CONSTANT && pad_mode != DSV_STFT_PAD_REFLECT) return fail(DSD_ERR_INVALID, "%s: pad_mode=%d (0 constant, 1 reflect)", who, pad_mode);
    if (pad_l < 0 || pad_r < 0 || pad_l > (1 << 20) || pad_r > (1 << 20)) return fail(DSD_ERR_INVALID, "%s: padding (%d, %d) must be in [0, 2^20]", who, pad_l, pad_r);
    if (pad_mode == DSV_STFT_PAD_REFLECT && (pad_l >= L || pad_r >= L))
        return fail(DSD_ERR_INVALID, "%s: reflect padding (%d, %d) must be smaller than the signal (L=%d)", who, pad_l, pad_r, L);
    const int64_t nF = dsv_stft_frames(L, n_fft, hop, pad_l, pad_r);
    if (nF < 1) return fail(DSD_ERR_INVALID, "%s: signal shorter than one frame (L=%d + padding %d + %d < n_fft=%d)", who, L, pad_l, pad_r, n_fft);
    if (nF > (1 << 30)) return fail(DSD_ERR_INVALID, "%s: too many frames (%lld)", who, (long long)nF);
    p = StftParams{};
    p.in = wav; p.basis = reinterpret_cast<const float4*>(basis); p.lengths = lengths;
    p.L = L; p.N = n_fft; p.hop = hop; p.pad_l = pad_l; p.pad_r = pad_r; p.reflect = pad_mode == DSV_STFT_PAD_REFLECT; p.nF = (int)nF;
    return DSD_OK;
}

// workgroups of few-frame calls split the row groups over grid.z until the chip has two rounds of work (rows are independent in MODE 0 / 2)
static unsigned stft_zsplit(unsigned gx, unsigned B, int n_fft, int GT) {
    const unsigned ngroups = (unsigned)((n_fft / 32 + 4 * GT - 1) / (4 * GT));
    const unsigned long long have = (unsigned long long)gx * B;
    const unsigned z = have >= 512 ? 1u : (unsigned)((512 + have - 1) / have);
    return z > ngroups ? ngroups : z;
}

extern "C" int dsv_stft(const float* wav, const int32_t* lengths, const float* fwd_basis, float* spec, int32_t* frames_out, int32_t B, int32_t L,
                        int32_t n_fft, int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode, int32_t subtract, float v, void* stream) {
    StftParams p;
    DSD_TRY(stft_fill(p, "dsv_stft", wav, lengths, fwd_basis, B, L, n_fft, hop, pad_l, pad_r, pad_mode));
    if (!spec) return fail(DSD_ERR_INVALID, "dsv_stft: null argument");
    if (subtract && !(v >= 0.0f && std::isfinite(v))) return fail(DSD_ERR_INVALID, "dsv_stft: the subtracted magnitude v=%g must be finite and >= 0", (double)v);
    p.out = spec; p.frames_out = frames_out; p.subtract = subtract ? 1 : 0; p.v = v;
    size_t lds;
    stft_plan(n_fft, hop, p.KC, p.RL, lds);
    if (first_on_device(700)) HIP_TRY(hipFuncSetAttribute((const void*)k_stft<0, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStftLdsBudget));
    const unsigned gx = (unsigned)((p.nF + kStftNF - 1) / kStftNF);
    hipLaunchKernelGGL((k_stft<0, 2>), dim3(gx, (unsigned)B, stft_zsplit(gx, (unsigned)B, n_fft, 2)), dim3(kStftThreads), lds, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_logmel(const float* wav, const int32_t* lengths, const float* fwd_basis, const float* mel_basis, float* out, float* linear,
                          int32_t* frames_out, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode,
                          int32_t clamp, int32_t M, float mag_eps, float floor, int32_t log10, void* stream) {
    StftParams p;
    DSD_TRY(stft_fill(p, "dsv_logmel", wav, lengths, fwd_basis, B, L, n_fft, hop, pad_l, pad_r, pad_mode));
    if (!mel_basis || !out) return fail(DSD_ERR_INVALID, "dsv_logmel: null argument");
    if (M < 1 || M > kStftMaxMel) return fail(DSD_ERR_INVALID, "dsv_logmel: M=%d mel bins must be in [1, %d]", M, kStftMaxMel);
    if (!(mag_eps >= 0.0f) || !(floor > 0.0f) || !std::isfinite(mag_eps) || !std::isfinite(floor))
        return fail(DSD_ERR_INVALID, "dsv_logmel: mag_eps=%g must be >= 0 and floor=%g > 0, both finite", (double)mag_eps, (double)floor);
    p.out = out; p.lin = linear; p.melb = mel_basis; p.frames_out = frames_out; p.clamp = clamp ? 1 : 0; p.M = M; p.mag_eps = mag_eps; p.floor = floor;
    p.log10 = log10 ? 1 : 0;
    size_t lds;
    stft_plan(n_fft, hop, p.KC, p.RL, lds);
    const size_t red = (size_t)kStftNF * ((size_t)((M + 31) / 32) * 32 + 1) * sizeof(float);      // the cross-wave mel sum reuses the window's LDS
    if (red > lds) lds = red;
    if (first_on_device(701)) HIP_TRY(hipFuncSetAttribute((const void*)k_stft<1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, kStftLdsBudget));
    const unsigned gx = (unsigned)((p.nF + kStftNF - 1) / kStftNF);
    hipLaunchKernelGGL((k_stft<1, 1>), dim3(gx, (unsigned)B, 1), dim3(kStftThreads), lds, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int64_t dsv_istft_workspace_floats(int32_t B, int64_t n_frames, int32_t n_fft) {
    if (B < 1 || n_frames < 1 || !stft_nfft_ok(n_fft)) return -1;
    return (int64_t)B * n_frames * n_fft;
}

extern "C" int dsv_istft(const float* spec, const int32_t* frame_counts, const float* inv_basis, float* workspace, float* wav, int32_t B,
                         int32_t n_frames, int32_t L_out, int32_t n_fft, int32_t hop, int32_t center, void* stream) {
    if (!spec || !inv_basis || !workspace || !wav) return fail(DSD_ERR_INVALID, "dsv_istft: null argument");
    if (!stft_nfft_ok(n_fft)) return fail(DSD_ERR_INVALID, "dsv_istft: n_fft=%d is not one of 256, 512, 1024, 2048", n_fft);
    if (hop < 1 || hop > n_fft) return fail(DSD_ERR_INVALID, "dsv_istft: hop=%d must be in [1, n_fft=%d]", hop, n_fft);
    if (B < 1 || B > 65535 || n_frames < 1 || n_frames > (1 << 30) || L_out < 1 || L_out > (1 << 30))
        return fail(DSD_ERR_INVALID, "dsv_istft: bad shape (B=%d in [1, 65535], n_frames=%d and L_out=%d in [1, 2^30])", B, n_frames, L_out);
    StftParams p{};
    p.in = spec; p.basis = reinterpret_cast<const float4*>(inv_basis); p.out = workspace; p.lengths = frame_counts;
    p.N = n_fft; p.hop = n_fft; p.nF = n_frames;
    size_t lds;
    stft_plan(n_fft, n_fft, p.KC, p.RL, lds);
    if (first_on_device(702)) HIP_TRY(hipFuncSetAttribute((const void*)k_stft<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStftLdsBudget));
    const unsigned gx = (unsigned)((n_frames + kStftNF - 1) / kStftNF);
    hipLaunchKernelGGL((k_stft<2, 2>), dim3(gx, (unsigned)B, stft_zsplit(gx, (unsigned)B, n_fft, 2)), dim3(kStftThreads), lds, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    IstftOlaParams q{};
    q.frames = workspace; q.wsq = inv_basis + (size_t)n_fft * n_fft; q.frame_counts = frame_counts; q.out = wav;
    q.nF = n_frames; q.N = n_fft; q.hop = hop; q.trim = center ? n_fft / 2 : 0; q.L_out = L_out;
    hipLaunchKernelGGL(k_istft_ola, dim3((unsigned)((L_out + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, q);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
