// fs2_regulate.hpp - the length regulator of FastSpeech2 (C ABI in include/dsf.h, dsf_length_regulate); included at the end of dsd.hip (one
// translation unit: shares fail(), HIP_TRY).
//
// What is computed, and where the reference computes it (paths relative to the reference root):
//   out2dur           modules/fastspeech/tts_modules.py:122-131 (DurationPredictor, dur_loss 'mse'): d = clamp(round(exp(y) - offset), min=0),
//                     every operation once in fp32 (exp through the device library, __ocml_exp_f32 - the function ATen's exp kernel calls;
//                     round = rintf, half to even);
//   LengthRegulator   modules/fastspeech/tts_modules.py:158-186: d = round(d.float() * alpha).long(), d = 0 on padded tokens, then
//                     mel2ph[t] = sum_j (j + 1) [cumsum_prev[j] <= t < cumsum[j]].  The intervals are disjoint, so the sum has one term at most:
//                     j + 1 for the first token whose inclusive running sum exceeds t (tokens of length 0 own no frame), 0 past the row's sum.
//
// k_fs_length_regulate: one workgroup per (1024-frame tile, utterance).  Each workgroup redoes the row's element-wise steps and its running sum
// in LDS (T_txt <= 4096 words; cheaper than a second launch or a grid-wide dependency), then each thread resolves two CONSECUTIVE frames per
// pass by binary search in LDS and writes them with one 16-byte store.  Workgroup (0, b) writes dur_out and mel_len.  Integers only after
// the element-wise step, fixed order, no atomics: two launches are bitwise equal.  Durations saturate at kRegMaxDur per token and the
// running sum at INT32_MAX (a saturating add of non-negative numbers is associative, so the scan's tree order does not matter).
#pragma once

namespace dsd {

constexpr int kRegMaxTxt = DSF_REGULATE_MAX_TXT;   // tokens per row: the running sums of one row live in one workgroup's LDS (16 KiB)
constexpr int kRegMaxDur = 1 << 20;                // frames per token
constexpr int kRegThreads = 256;
constexpr int kRegTile = 1024;                     // frames per workgroup: two passes of 256 threads x 2 frames
constexpr unsigned kRegSumCap = 0x7fffffffu;

struct FsRegulateParams {
    const long long* dur;           // [B][T_txt] integer durations, or null
    const float* logdur;            // [B][T_txt] the duration predictor's output, or null (exactly one of the two)
    const unsigned char* padding;   // [B][T_txt] nonzero = padded token, or null
    long long* dur_out;             // [B][T_txt] out2dur's result (logdur form only), or null
    long long* mel2ph;              // [B][T_out], or null
    int* mel_len;                   // [B] the row's sum (not clipped to T_out), or null
    int T_txt, T_out, vec;          // vec: rows of mel2ph are 16-byte aligned (two frames per store)
    float offset, alpha;
};

__device__ __forceinline__ unsigned reg_sat_add(unsigned a, unsigned b) {       // a, b <= kRegSumCap: a + b cannot wrap 32 bits
    const unsigned s = a + b;
    return s > kRegSumCap ? kRegSumCap : s;
}

// first j in [lo, n) with cum[j] > t; n if there is none
__device__ __forceinline__ int reg_upper(const unsigned* cum, int lo, int n, unsigned t) {
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kRegThreads) k_fs_length_regulate(FsRegulateParams p) {
    __shared__ unsigned cum[kRegMaxTxt];
    __shared__ unsigned wave_tot[kRegThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.y, n = p.T_txt;
    const size_t row = (size_t)b * n;
    const bool first = blockIdx.x == 0;

    // element-wise: out2dur (or the caller's integers), alpha, padding -> cum[i] = d_i (coalesced)
    for (int i = tid; i < n; i += kRegThreads) {
        float d;
        if (p.logdur) {
            const float e = expf(p.logdur[row + i]);
            d = fmaxf(rintf(e - p.offset), 0.0f);                                // NaN -> 0 (fmaxf returns the other operand)
            d = fminf(d, (float)kRegMaxDur);
            if (first && p.dur_out) p.dur_out[row + i] = (long long)d;
        } else {
            long long v = p.dur[row + i];
            v = v < 0 ? 0 : (v > kRegMaxDur ? kRegMaxDur : v);
            d = (float)v;
        }
        d = fminf(rintf(d * p.alpha), (float)kRegMaxDur);
        if (p.padding && p.padding[row + i]) d = 0.0f;
        cum[i] = (unsigned)d;
    }
    __syncthreads();

    // inclusive running sum: thread tid owns the `per` consecutive tokens from tid * per; serial inside, wave64 scan of the thread totals,
    // then the four wave totals
    const int per = (n + kRegThreads - 1) / kRegThreads;
    const int i0 = tid * per, i1 = min(i0 + per, n);
    unsigned tot = 0;
    for (int i = i0; i < i1; ++i) { tot = reg_sat_add(tot, cum[i]); cum[i] = tot; }
    const int lane = tid & 63, wave = tid >> 6;
    unsigned inc = tot;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o, 64);
        if (lane >= o) inc = reg_sat_add(inc, up);
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    const unsigned up1 = __shfl_up(inc, 1, 64);
    unsigned before = lane ? up1 : 0u;                                           // exclusive prefix of the thread totals inside the wave
    for (int w = 0; w < wave; ++w) before = reg_sat_add(before, wave_tot[w]);
    for (int i = i0; i < i1; ++i) cum[i] = reg_sat_add(cum[i], before);
    __syncthreads();

    const unsigned total = cum[n - 1];
    if (first && tid == 0 && p.mel_len) p.mel_len[b] = (int)total;
    if (!p.mel2ph) return;

    long long* out = p.mel2ph + (size_t)b * p.T_out;
    const int base = blockIdx.x * kRegTile;
    for (int t = base + tid * 2; t < min(base + kRegTile, p.T_out); t += kRegThreads * 2) {
        const int j0 = reg_upper(cum, 0, n, (unsigned)t);
        const long long m0 = j0 < n ? j0 + 1 : 0;
        if (t + 1 < p.T_out) {
            const int j1 = reg_upper(cum, j0, n, (unsigned)t + 1u);
            const long long m1 = j1 < n ? j1 + 1 : 0;
            if (p.vec) {
                *reinterpret_cast<longlong2*>(out + t) = make_longlong2(m0, m1);
            } else {
                out[t] = m0;
                out[t + 1] = m1;
            }
        } else {
            out[t] = m0;
        }
    }
}

}  // namespace dsd

extern "C" int dsf_length_regulate(const int64_t* dur, const float* logdur, float offset, const uint8_t* dur_padding, float alpha, int64_t* dur_out,
                                   int64_t* mel2ph, int32_t* mel_len, int32_t B, int32_t T_txt, int32_t T_out, void* stream) {
    if ((dur != nullptr) == (logdur != nullptr))
        return fail(DSD_ERR_INVALID, "dsf_length_regulate: exactly one of dur and logdur must be given");
    if (!(alpha > 0.0f) || std::isinf(alpha)) return fail(DSD_ERR_INVALID, "dsf_length_regulate: alpha must be positive and finite (got %g)", (double)alpha);
    if (B < 1 || B > 65535 || T_txt < 1 || T_out < 1 || T_out > (1 << 30))
        return fail(DSD_ERR_INVALID, "dsf_length_regulate: bad shape (B=%d in [1, 65535], T_txt=%d >= 1, T_out=%d in [1, 2^30])", B, T_txt, T_out);
    if (T_txt > DSF_REGULATE_MAX_TXT)
        return fail(DSD_ERR_INVALID, "dsf_length_regulate: T_txt=%d above the supported maximum %d (DSF_REGULATE_MAX_TXT)", T_txt, DSF_REGULATE_MAX_TXT);
    if (!mel2ph && !mel_len && !(dur_out && logdur)) return fail(DSD_ERR_INVALID, "dsf_length_regulate: no output asked for (mel2ph, mel_len, dur_out)");
    if (logdur && std::isnan(offset)) return fail(DSD_ERR_INVALID, "dsf_length_regulate: offset is NaN");
    FsRegulateParams p{};
    p.dur = (const long long*)dur; p.logdur = logdur; p.padding = dur_padding; p.dur_out = logdur ? (long long*)dur_out : nullptr;
    p.mel2ph = (long long*)mel2ph; p.mel_len = mel_len; p.T_txt = T_txt; p.T_out = T_out; p.offset = offset; p.alpha = alpha;
    p.vec = (T_out % 2 == 0 && ((uintptr_t)mel2ph & 15) == 0) ? 1 : 0;
    const unsigned tiles = mel2ph ? (unsigned)((T_out + kRegTile - 1) / kRegTile) : 1u;
    hipLaunchKernelGGL(k_fs_length_regulate, dim3(tiles, (unsigned)B), dim3(kRegThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}
