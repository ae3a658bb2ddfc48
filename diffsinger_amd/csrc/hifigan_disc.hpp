// hifigan_disc.hpp - gfx950 kernels and host side of the HiFi-GAN multi-scale discriminator's pooling (modules/hifigan/hifigan.py:304-307, :316-317:
// AvgPool1d(4, 2, padding=1) applied cumulatively to y and y_hat in front of the second and third DiscriminatorS), forward and backward.  C ABI in
// include/dsv.h, section "HiFi-GAN scale discriminator"; included at the end of dsd.hip.  Outputs are rows [R][LS(L)] float32 and both kernels leave
// [L, LS) of them at zero - the contract of the generator's operators; the input's rows lie `ld` >= L floats apart and nothing is read beyond
// sample L of a row, so a dense [R][L] tensor goes in without a padding pass.  Plain vector-ALU kernels, one thread per output sample, a fixed
// order of additions: two calls are bitwise equal.
#pragma once
#include "voc_kernels.hpp"
#include "voc_train_host.hpp"

namespace dsd {

// out[q] = (x[2 q - 1] + x[2 q] + x[2 q + 1] + x[2 q + 2]) / 4, zero outside [0, L): count_include_pad, the divisor is always 4
__global__ __launch_bounds__(256) void k_hgd_avgpool(const float* __restrict__ x, float* __restrict__ out, int L, long long ld, int Lo, int LSo) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= LSo) return;
    float v = 0.f;
    if (q < Lo) {
        const float* r = x + (size_t)blockIdx.y * ld;
        const int n = 2 * q - 1;
        const float x0 = n >= 0 ? r[n] : 0.f, x1 = r[n + 1], x2 = n + 2 < L ? r[n + 2] : 0.f, x3 = n + 3 < L ? r[n + 3] : 0.f;
        v = (((x0 + x1) + x2) + x3) * 0.25f;
    }
    out[(size_t)blockIdx.y * LSo + q] = v;
}

// dx[n] = (g[(n + 1) / 2 - 1] + g[(n + 1) / 2]) / 4, the outputs whose windows 2 q - 1 .. 2 q + 2 hold n
__global__ __launch_bounds__(256) void k_hgd_avgpool_bwd(const float* __restrict__ g, float* __restrict__ dx, int L, int LS, int Lo, long long ld) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= LS) return;
    float v = 0.f;
    if (n < L) {
        const float* r = g + (size_t)blockIdx.y * ld;
        const int qh = (n + 1) >> 1, ql = qh - 1;
        const float g0 = ql >= 0 && ql < Lo ? r[ql] : 0.f, g1 = qh < Lo ? r[qh] : 0.f;
        v = (g0 + g1) * 0.25f;
    }
    dx[(size_t)blockIdx.y * LS + n] = v;
}

}  // namespace dsd

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
extern "C" int32_t dsv_hgd_pool_samples(int32_t L) { return L < 2 ? -1 : L / 2; }

extern "C" int dsv_hgd_avgpool(const float* x, float* out, int64_t R, int32_t L, int64_t ld_x, void* stream) {
    const int Lo = L / 2, LSo = L >= 2 ? voc_ls(Lo) : 0;
    DSD_TRY(voc_check_pool_rows("dsv_hgd_avgpool", x, out, R, L, ld_x, L, LSo));
    hipLaunchKernelGGL(k_hgd_avgpool, dim3((unsigned)((LSo + 255) / 256), (unsigned)R), dim3(256), 0, (hipStream_t)stream, x, out, L, (long long)ld_x, Lo,
                       LSo);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgd_avgpool_backward(const float* g, float* dx, int64_t R, int32_t L, int64_t ld_g, void* stream) {
    const int Lo = L / 2, LS = L >= 2 ? voc_ls(L) : 0;
    DSD_TRY(voc_check_pool_rows("dsv_hgd_avgpool_backward", g, dx, R, L, ld_g, Lo, LS));
    hipLaunchKernelGGL(k_hgd_avgpool_bwd, dim3((unsigned)((LS + 255) / 256), (unsigned)R), dim3(256), 0, (hipStream_t)stream, g, dx, L, LS, Lo,
                       (long long)ld_g);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
