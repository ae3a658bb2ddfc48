// voc_train_host.hpp - the host checks the vocoder-training entry points share (pwg_disc_abi.hpp, pwg_train_abi.hpp, hifigan_train_abi.hpp,
// voc_stft_loss_abi.hpp); included behind dsd.hip's fail().  The messages are part of the ABI's behaviour: tests assert on them.
#pragma once

// B batch rows of L samples: what every grid and every 32-bit index of these kernels holds
static bool voc_shape_ok(int B, int L) { return B >= 1 && B <= 65535 && L >= 1 && L <= (1 << 30); }

// `len` names the length in the message: L, or T in the discriminator's
static int voc_check_shape(const char* who, int B, int L, char len = 'L') {
    if (!voc_shape_ok(B, L)) return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d in [1, 65535], %c=%d in [1, 2^30])", who, B, len, L);
    return DSD_OK;
}

// a workspace that kernels read and write as float64; `note` is the message's parenthesis
static int voc_check_f64_workspace(const char* who, const void* ptr, const char* note = "float64 sums") {
    if ((uintptr_t)ptr & 7) return fail(DSD_ERR_INVALID, "%s: the workspace must be aligned to 8 bytes (%s)", who, note);
    return DSD_OK;
}

// the leaky ReLU's slope
static int voc_check_slope(const char* who, float slope) {
    if (!(slope > 0.f && slope < 1.f)) return fail(DSD_ERR_INVALID, "%s: negative_slope=%g must be in (0, 1)", who, (double)slope);
    return DSD_OK;
}

// C channels of an edge layer (1 -> C or C -> 1): C is a grid dimension
static int voc_check_grid_channels(const char* who, int C) {
    if (C < 1 || C > 65535) return fail(DSD_ERR_INVALID, "%s: C=%d must be in [1, 65535]", who, C);
    return DSD_OK;
}

// rows of T samples `ld` floats apart
static int voc_check_row_stride(const char* who, int64_t ld, int T) {
    if (ld < T || ld > ((int64_t)1 << 31)) return fail(DSD_ERR_INVALID, "%s: row stride %lld must be in [T=%d, 2^31]", who, (long long)ld, T);
    return DSD_OK;
}

// splits of `len` samples that cover L
static int voc_splits(int L, int len) { return (L + len - 1) / len; }

// B planes of [H][p] positions of the period discriminator: B and B * p bound the grids, B * H * p <= 2^30 every 32-bit position index
static bool voc_period_shape_ok(int B, int H, int p) {
    return B >= 1 && H >= 1 && p >= 1 && p <= 64 && (int64_t)B * p <= 65535 && (int64_t)B * H * p <= ((int64_t)1 << 30);
}
static int voc_check_period_shape(const char* who, int B, int H, int p) {
    if (!voc_period_shape_ok(B, H, p))
        return fail(DSD_ERR_INVALID, "%s: bad shape (B=%d >= 1, H=%d >= 1, period=%d in [1, 64], B * period <= 65535, B * H * period <= 2^30)", who, B, H, p);
    return DSD_OK;
}

// an input range [in, in + n_in) and an output range [out, out + n_out) of floats that must not overlap
static int voc_check_disjoint(const char* who, const float* in, int64_t n_in, const float* out, int64_t n_out) {
    if (in < out + n_out && out < in + n_in) return fail(DSD_ERR_INVALID, "%s: input and output overlap", who);
    return DSD_OK;
}

// R rows pooled by AvgPool1d(4, 2, 1) from L samples: `in` holds R rows `ld` floats apart of which `in_len` are read, `out` R rows of `out_ld`
// floats; the two ranges must not overlap
static int voc_check_pool_rows(const char* who, const float* in, const float* out, int64_t R, int L, int64_t ld, int in_len, int out_ld) {
    if (!in || !out) return fail(DSD_ERR_INVALID, "%s: null argument", who);
    if (R < 1 || R > 65535 || L < 2 || L > (1 << 30) || ld < in_len || ld > ((int64_t)1 << 31))
        return fail(DSD_ERR_INVALID, "%s: bad shape (R=%lld in [1, 65535], L=%d in [2, 2^30], row stride %lld in [%d, 2^31])", who, (long long)R, L,
                    (long long)ld, in_len);
    const float* in_end = in + (R - 1) * ld + in_len;
    const float* out_end = out + R * (int64_t)out_ld;
    if (in < out_end && out < in_end) return fail(DSD_ERR_INVALID, "%s: input and output overlap", who);
    return DSD_OK;
}
