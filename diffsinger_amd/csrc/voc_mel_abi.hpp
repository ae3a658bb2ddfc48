// voc_mel_abi.hpp - host side of the mel loss (C ABI in include/dsv.h, section "Mel loss"; kernels in voc_mel.hpp); included at the end of
// dsd.hip behind voc_stft_abi.hpp (shares stft_nfft_ok, stft_fill, stft_plan, stft_zsplit).  Every entry point validates on the host and
// refuses with DSD_ERR_INVALID before any launch; nothing allocates or synchronises.
#include "voc_mel.hpp"

// site id of first_on_device in this file: 704.  It sets the dynamic-LDS attribute of k_stft<0, 2> - the SAME function object site 700 (dsv_stft,
// voc_stft_abi.hpp) sets: both stay, because either entry point can be the first caller of the kernel on a device.

extern "C" int dsv_mel_spectrum(const float* wav, const float* fwd_basis, float* spec, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t pad_l,
                                int32_t pad_r, int32_t pad_mode, int32_t clamp, void* stream) {
    StftParams p;
    DSD_TRY(stft_fill(p, "dsv_mel_spectrum", wav, nullptr, fwd_basis, B, L, n_fft, hop, pad_l, pad_r, pad_mode));
    if (!spec) return fail(DSD_ERR_INVALID, "dsv_mel_spectrum: null argument");
    p.out = spec; p.clamp = clamp ? 1 : 0;
    size_t lds;
    stft_plan(n_fft, hop, p.KC, p.RL, lds);
    if (first_on_device(704)) HIP_TRY(hipFuncSetAttribute((const void*)k_stft<0, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, kStftLdsBudget));
    const unsigned gx = (unsigned)((p.nF + kStftNF - 1) / kStftNF);
    hipLaunchKernelGGL((k_stft<0, 2>), dim3(gx, (unsigned)B, stft_zsplit(gx, (unsigned)B, n_fft, 2)), dim3(kStftThreads), lds, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

// [a, a + na) and [b, b + nb) floats
static bool mel_ranges_overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

// the arguments both heads share; fills everything of `p` but the pointers
static int mel_head_check(MelHeadParams& p, const char* who, int32_t B, int32_t T, int32_t n_fft, int32_t M, float mag_eps, float floor, int32_t log10) {
    if (!stft_nfft_ok(n_fft)) return fail(DSD_ERR_INVALID, "%s: n_fft=%d is not one of 256, 512, 1024, 2048", who, n_fft);
    if (M < 1 || M > kStftMaxMel) return fail(DSD_ERR_INVALID, "%s: M=%d mel bins must be in [1, %d]", who, M, kStftMaxMel);
    if (B < 1 || B > 65535 || T < 1 || T > (1 << 30)) return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d in [1, 65535], T=%d in [1, 2^30])", who, B, T);
    if (!(mag_eps >= 0.0f) || !(floor > 0.0f) || !std::isfinite(mag_eps) || !std::isfinite(floor))
        return fail(DSD_ERR_INVALID, "%s: mag_eps=%g must be >= 0 and floor=%g > 0, both finite", who, (double)mag_eps, (double)floor);
    p = MelHeadParams{};
    p.T = T; p.n_bins = n_fft / 2 + 1; p.M = M; p.log10 = log10 ? 1 : 0; p.mag_eps = mag_eps; p.floor = floor;
    return DSD_OK;
}

extern "C" int dsv_mel_head(const float* spec, const float* mel_basis, float* out, float* mel, int32_t B, int32_t T, int32_t n_fft, int32_t M,
                            float mag_eps, float floor, int32_t log10, void* stream) {
    if (!spec || !mel_basis || !out || !mel) return fail(DSD_ERR_INVALID, "dsv_mel_head: null argument");
    MelHeadParams p;
    DSD_TRY(mel_head_check(p, "dsv_mel_head", B, T, n_fft, M, mag_eps, floor, log10));
    if ((uintptr_t)spec & 7) return fail(DSD_ERR_INVALID, "dsv_mel_head: the spectrum must be aligned to 8 bytes (it is read as (re, im) pairs)");
    const int64_t ns = (int64_t)B * p.n_bins * T * 2, nw = (int64_t)M * p.n_bins, no = (int64_t)B * T * M;
    if (mel_ranges_overlap(out, no, spec, ns) || mel_ranges_overlap(out, no, mel_basis, nw) || mel_ranges_overlap(mel, no, spec, ns) ||
        mel_ranges_overlap(mel, no, mel_basis, nw) || mel_ranges_overlap(out, no, mel, no))
        return fail(DSD_ERR_INVALID, "dsv_mel_head: an output overlaps an input or the other output");
    p.S = reinterpret_cast<const float2*>(spec); p.W = mel_basis; p.out = out; p.mel = mel;
    hipLaunchKernelGGL(k_mel_head, dim3((unsigned)((T + kMelNF - 1) / kMelNF), (unsigned)B, (unsigned)((M + 31) / 32)), dim3(kMelThreads), 0,
                       (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_mel_head_backward(const float* spec, const float* mel_basis, const float* grad_out, const float* mel, float* G, int32_t B, int32_t T,
                                     int32_t n_fft, int32_t M, float mag_eps, float floor, int32_t log10, void* stream) {
    if (!spec || !mel_basis || !grad_out || !mel || !G) return fail(DSD_ERR_INVALID, "dsv_mel_head_backward: null argument");
    MelHeadParams p;
    DSD_TRY(mel_head_check(p, "dsv_mel_head_backward", B, T, n_fft, M, mag_eps, floor, log10));
    if (((uintptr_t)spec | (uintptr_t)G) & 7)
        return fail(DSD_ERR_INVALID, "dsv_mel_head_backward: the spectrum and its gradient must be aligned to 8 bytes ((re, im) pairs)");
    const int64_t ns = (int64_t)B * p.n_bins * T * 2, nw = (int64_t)M * p.n_bins, no = (int64_t)B * T * M;
    if (mel_ranges_overlap(G, ns, spec, ns) || mel_ranges_overlap(G, ns, mel_basis, nw) || mel_ranges_overlap(G, ns, grad_out, no) ||
        mel_ranges_overlap(G, ns, mel, no))
        return fail(DSD_ERR_INVALID, "dsv_mel_head_backward: the output G overlaps an input");
    p.S = reinterpret_cast<const float2*>(spec); p.W = mel_basis; p.g = grad_out; p.mel_in = mel; p.G = reinterpret_cast<float2*>(G);
    const unsigned ntiles = (unsigned)((p.n_bins + 31) / 32);
    hipLaunchKernelGGL(k_mel_head_bwd, dim3((unsigned)((T + kMelNF - 1) / kMelNF), (unsigned)B, (ntiles + 3) / 4), dim3(kMelThreads), 0,
                       (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_mel_clamp_backward(const float* x, const float* dx_in, float* dx_out, int64_t n, void* stream) {
    if (!x || !dx_in || !dx_out) return fail(DSD_ERR_INVALID, "dsv_mel_clamp_backward: null argument");
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(DSD_ERR_INVALID, "dsv_mel_clamp_backward: bad shape (n=%lld floats must be in [1, 2^40])", (long long)n);
    if (mel_ranges_overlap(dx_out, n, x, n) || (dx_out != dx_in && mel_ranges_overlap(dx_out, n, dx_in, n)))
        return fail(DSD_ERR_INVALID, "dsv_mel_clamp_backward: dx_out overlaps x, or dx_in other than in place");
    const int64_t want = (n + 255) / 256;
    hipLaunchKernelGGL(k_mel_clamp_bwd, dim3((unsigned)(want > 16384 ? 16384 : want)), dim3(256), 0, (hipStream_t)stream, x, dx_in, dx_out, (long long)n);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
