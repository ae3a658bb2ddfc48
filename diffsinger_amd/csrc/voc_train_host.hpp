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

// splits of `len` samples that cover L
static int voc_splits(int L, int len) { return (L + len - 1) / len; }
