// voc_stft.hpp - the short-time Fourier transform family of the vocoder classes (C ABI in include/dsv.h, section "STFT"; host side in
// voc_stft_abi.hpp): framed real DFT, its inverse with overlap-add, the spectral-subtraction post-filter and the log-mel analysis.
//
// What is computed, and where the reference computes it (paths relative to the reference root):
//   stft / denoise   vocoders/vocoder_utils.py:7-15 (librosa.stft -> |S| - v clipped at 0, phase kept -> librosa.istft), called from
//                    vocoders/hifigan.py:67-68;
//   log-mel (pwg)    data_gen/tts/data_gen_utils.py:122-134 (librosa.stft pad_mode='constant', |S|, mel_basis @ |S|, log10(max(eps, .)));
//   log-mel (hifigan) modules/hifigan/mel_utils.py:59-76 (clamp, reflect padding (n_fft - hop) / 2, torch.stft center=False,
//                    sqrt(re^2 + im^2 + 1e-9), mel_basis @ ., log(clamp(., min=1e-5))).
//
// THE DFT IS A MATRIX PRODUCT on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), frames are the columns:
//     D[row][frame] = sum_n  A[row][n] * x[frame * hop + n]
// A = the precomputed basis, n_fft rows x n_fft columns, the analysis window folded in, each entry the float32 rounding of the float64 value
// with the angle reduced exactly ((k n) mod n_fft in integers):
//     row 0      = w[n]                         (Re of bin 0;      Im of bin 0 is identically 0 and has no row)
//     row 1      = w[n] cos(pi n)               (Re of bin n_fft/2; its Im is identically 0: it takes the slot bin 0's Im would have)
//     row 2k     = w[n] cos(2 pi k n / n_fft)   (Re of bin k, 1 <= k < n_fft/2)
//     row 2k + 1 = -w[n] sin(2 pi k n / n_fft)  (Im of bin k)
// so the product has exactly n_fft rows (n_fft / 32 MFMA row tiles, none padded) and - by the C/D map of the instruction, lane (j, h),
// register r holds row (r & 3) + 8 (r >> 2) + 4 h - the real and the imaginary part of a bin are registers 2q and 2q + 1 of ONE lane: the
// magnitude, the spectral subtraction and the mel product need no exchange between lanes.
// The inverse is the same product with the roles swapped: A = inverse basis [n][c] (synthesis window, 1 / n_fft and the factor 2 of the
// interior bins folded in; column c in the row order above), "signal" = the spectrum, frame stride n_fft.
//
// One workgroup (256 threads, 4 waves) owns 64 consecutive frames of one utterance and ALL rows; wave w takes the row tiles w, w + 4, ...
// and two 32-frame column blocks per A fragment.  The A fragments stream from memory (packed in fragment order: one 16-byte load per lane
// per four k-steps, 1 KiB per wave, coalesced; the basis is shared by every workgroup and lives in L2 / MALL).  The frames are NOT
// materialised: the workgroup stages the sample window of its 64 frames once in LDS - padding (zeros or reflection), the clamp and the row's
// valid length are index arithmetic of that staging - and reads the overlapping frames from it.  LDS layout: rows of RL = min(hop, KC)
// samples at a stride of RL + 2 floats, row i starting at sample (f0 + i) * hop + n0 of the padded signal; sample n of frame f sits in row
// f + n / RL.  With RL a multiple of 64 the 64 lanes of a B read (32 frames x 2 consecutive samples) hit 64 different banks (2 j + h).
// When the window of all n_fft samples does not fit the LDS budget (72 KiB: room for two workgroups per CU, though as built the float64
// running totals put every instantiation above 256 registers, one workgroup of four waves per CU) - large hops, and always the inverse -
// the contraction runs in chunks of KC samples (a power of two), the accumulators of GT row tiles per wave staying in registers across the
// chunks of a group.
//
// Epilogues, all from the accumulators:
//   MODE 0  spectrum [B][n_bins][n_frames][2] (re, im interleaved - the memory of a torch complex64 tensor [B][n_bins][n_frames], the layout
//           torch.stft returns), optionally S' = S * max(|S| - v, 0) / |S| (0 where |S| = 0); the unfiltered spectrum is never written.
//   MODE 1  mag = sqrt(re^2 + im^2 + mag_eps); mel += basis[M][bins of this tile] * mag as a second MFMA product whose B operand IS the
//           accumulator tile (the magnitudes of a lane are rows of the product's k index: no LDS, no lane movement); the four waves' partial
//           mel tiles are summed through LDS in the fixed order ((w0 + w1) + w2) + w3; out = log(max(mel, floor)) - natural or base 10, evaluated
//           in float64 and rounded once - written [B][n_frames][M].  FRAMES AT OR BEYOND A ROW'S VALID COUNT (from `lengths`) ARE WRITTEN AS
//           EXACTLY 0, the library's padding value for mels (the linear magnitude and the spectrum of MODE 0 likewise).
//   MODE 2  (inverse) windowed frames [B][n_frames][n_fft] to a workspace; a second launch (k_istft_ola) overlap-adds them as a GATHER: every
//           output sample adds its at most ceil(n_fft / hop) contributing frame values in ascending frame order - the order of the host loop of
//           diffsinger_amd.vocoder.denoise - forms its own window sum-of-squares the same way and divides where that exceeds FLT_MIN.
//           TWO LAUNCHES, not one: a fused workgroup would need its 64 frames plus a halo of n_fft / hop - 1 frames per side as [frames][n_fft]
//           in LDS (70 x 1024 x 4 B = 280 KiB at the shipped shape) - more than a CU has; the intermediate is 4 KiB per frame and stays in L2 / MALL.
// No atomics, every sum in a fixed order: two calls are bitwise equal.
#pragma once

#include <float.h>

namespace dsd {

constexpr int kStftThreads = 256;
constexpr int kStftNF = 64;                   // frames per workgroup: two 32-column MFMA blocks
constexpr int kStftLdsBudget = 72 * 1024;     // bytes of staged samples per workgroup
constexpr int kStftMaxMel = 128;
constexpr int kStftSeg = 2;                   // float4 A loads (of four k-steps of two samples each) per fp32 summation chain: 16 samples

typedef double f64x16 __attribute__((ext_vector_type(16)));

struct StftParams {
    const float* in;          // MODE 0 / 1: waveform [B][L]; MODE 2: spectrum [B][n_bins][nF][2]
    const float4* basis;      // packed A operand (k_stft_make_basis)
    float* out;               // MODE 0: spectrum; MODE 1: log-mel [B][nF][M]; MODE 2: windowed frames [B][nF][N]
    float* lin;               // MODE 1: linear magnitude [B][nF][n_bins], or null
    const float* melb;        // MODE 1: mel basis [M][n_bins]
    const int* lengths;       // [B] valid samples per row (MODE 0 / 1) / valid frames per row (MODE 2), or null
    int* frames_out;          // MODE 0 / 1: [B] valid frames per row, or null
    int L, N, hop, pad_l, pad_r, reflect, clamp, nF;
    int KC, RL, M, log10, subtract;
    float v, mag_eps, floor;
};

// valid frames of a row of `len` samples
__device__ __forceinline__ int stft_row_frames(int len, const StftParams& p) {
    const long long tot = (long long)len + p.pad_l + p.pad_r;
    if (len < 1 || tot < p.N) return 0;
    const long long nf = 1 + (tot - p.N) / p.hop;
    return (int)(nf < p.nF ? nf : p.nF);
}

// sample `pos` of the padded signal of a row with `len` valid samples (index arithmetic only: there is no padded copy)
__device__ __forceinline__ float stft_sample(const float* x, long long pos, int len, const StftParams& p) {
    long long u = pos - p.pad_l;
    if (u >= (long long)len + p.pad_r) return 0.0f;
    if (u < 0 || u >= len) {
        if (!p.reflect) return 0.0f;
        u = u < 0 ? -u : 2LL * (len - 1) - u;
        if (u < 0 || u >= len) return 0.0f;
    }
    float s = x[u];
    if (p.clamp) s = fminf(fmaxf(s, -1.0f), 1.0f);
    return s;
}

template <int MODE, int GT>
__global__ void __launch_bounds__(kStftThreads) k_stft(StftParams p) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, f0 = blockIdx.x * kStftNF;
    const int N = p.N, KC = p.KC, RL = p.RL, LD = RL + 2, nchunks = N / KC, n_bins = N / 2 + 1, nF = p.nF;
    const int nrows = kStftNF - 1 + (KC + RL - 1) / RL;
    const int ntiles = N / 32, ngroups = (ntiles + 4 * GT - 1) / (4 * GT);

    int len = 0, nfb;
    if (MODE == 2) {
        nfb = p.lengths ? min(max(p.lengths[b], 0), nF) : nF;
    } else {
        len = p.lengths ? min(max(p.lengths[b], 0), p.L) : p.L;
        nfb = stft_row_frames(len, p);
        if (p.frames_out && blockIdx.x == 0 && blockIdx.z == 0 && tid == 0) p.frames_out[b] = nfb;
    }
    const float* xin = MODE == 2 ? p.in + (size_t)b * n_bins * nF * 2 : p.in + (size_t)b * p.L;

    f32x16 mel[MODE == 1 ? 4 : 1][2];
    if constexpr (MODE == 1) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) { mel[mt][0] = f32x16(0.0f); mel[mt][1] = f32x16(0.0f); }
    }
    const int Mt = MODE == 1 ? (p.M + 31) / 32 : 0;

    bool staged = false;
    for (int grp = blockIdx.z; grp < ngroups; grp += gridDim.z) {
        f64x16 acc[GT][2];                                                     // running totals of the fp32 chains, in float64 (see the main loop)
#pragma unroll
        for (int s = 0; s < GT; ++s) { acc[s][0] = f64x16(0.0); acc[s][1] = f64x16(0.0); }

        for (int ch = 0; ch < nchunks; ++ch) {
            const int n0 = ch * KC;
            if (nchunks > 1 || !staged) {
                if (staged) __syncthreads();                               // every wave is done reading the previous chunk
                if (MODE == 2) {
                    // row i = frame f0 + i, column r = spectrum slot n0 + r; frames fastest (8-byte stride in memory)
                    for (int idx = tid; idx < kStftNF * KC; idx += kStftThreads) {
                        const int i = idx & (kStftNF - 1), r = idx / kStftNF, c = n0 + r, f = f0 + i;
                        const int bin = c == 1 ? N / 2 : (c >> 1), part = c == 1 ? 0 : (c & 1);
                        lds[i * LD + r] = f < nfb ? xin[((size_t)bin * nF + f) * 2 + part] : 0.0f;
                    }
                } else {
                    const long long base = (long long)f0 * p.hop + n0;
                    for (int idx = tid; idx < nrows * RL; idx += kStftThreads) {
                        const int i = idx / RL, r = idx - i * RL;
                        lds[i * LD + r] = stft_sample(xin, base + (long long)i * p.hop + r, len, p);
                    }
                }
                __syncthreads();
                staged = true;
            }
#pragma unroll
            for (int s = 0; s < GT; ++s) {
                const int rt = (grp * GT + s) * 4 + wave;
                if (rt < ntiles) {
                    const float4* A = p.basis + ((size_t)rt * (N / 8) + n0 / 8) * 64 + lane;
                    const int nkq = KC / 8;
                    int r = h, addr = j * LD + h;
                    while (r >= RL) { r -= RL; addr += 2; }
                    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    float4 a0 = A[0], a1 = nkq > 1 ? A[64] : zero4;
                    // blocked summation: the MFMA accumulates fp32 chains of 16 samples (kStftSeg A loads) in c0 / c1; the chains' totals are added
                    // to the tile's running sum in FLOAT64 on the vector pipe (32 conversions + 32 additions per 16 MFMAs).  A k-ordered fp32 chain
                    // rounds every partial sum at ITS magnitude, and the partial sums of a DFT bin wander far above a small final value: one fp32
                    // chain over n_fft samples measured 2.4 x the error of a float32 matmul on the CPU, 64-sample chains with fp32 totals 0.6 - 3.4 x
                    f32x16 c0 = f32x16(0.0f), c1 = f32x16(0.0f);
                    for (int kq = 0; kq < nkq; ++kq) {
                        const float4 a2 = kq + 2 < nkq ? A[(size_t)(kq + 2) * 64] : zero4;
                        const float av[4] = {a0.x, a0.y, a0.z, a0.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float b0 = lds[addr], b1 = lds[addr + 32 * LD];
                            c0 = mfma32(av[e], b0, c0);
                            c1 = mfma32(av[e], b1, c1);
                            r += 2; addr += 2;
                            while (r >= RL) { r -= RL; addr += 2; }
                        }
                        a0 = a1; a1 = a2;
                        if ((kq & (kStftSeg - 1)) == kStftSeg - 1 || kq == nkq - 1) {
                            acc[s][0] += __builtin_convertvector(c0, f64x16); acc[s][1] += __builtin_convertvector(c1, f64x16);
                            c0 = f32x16(0.0f); c1 = f32x16(0.0f);
                        }
                    }
                }
            }
        }

        // epilogue of the group's row tiles
#pragma unroll
        for (int s = 0; s < GT; ++s) {
            const int rt = (grp * GT + s) * 4 + wave;
            if (rt >= ntiles) continue;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const int f = f0 + cb * 32 + j;
                const bool inbuf = f < nF, valid = f < nfb;
                const f32x16 c = __builtin_convertvector(acc[s][cb], f32x16);
                if constexpr (MODE == 2) {
                    // inverse basis rows are permuted so that a lane holds 16 consecutive samples: register 4 g + q = sample rt * 32 + 16 h + 4 g + q
                    if (inbuf) {
                        float4* o = reinterpret_cast<float4*>(p.out + ((size_t)b * nF + f) * N + rt * 32 + 16 * h);
#pragma unroll
                        for (int g = 0; g < 4; ++g) o[g] = make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
                    }
                } else {
                    float mag[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {                           // q = 2 g + pp: bin rt * 16 + 4 g + 2 h + pp
                        const int g = q >> 1, pp = q & 1;
                        const int bin = rt * 16 + 4 * g + 2 * h + pp;
                        float re = c[4 * g + 2 * pp], im = c[4 * g + 2 * pp + 1];
                        const bool dc = bin == 0;                           // (re of bin 0, re of bin N / 2) share this pair
                        float nyq = im;
                        if (dc) im = 0.0f;
                        if constexpr (MODE == 0) {
                            if (p.subtract) {
                                const float m = sqrtf(re * re + im * im);
                                const float sc = m > 0.0f ? fmaxf(m - p.v, 0.0f) / m : 0.0f;
                                re *= sc; im *= sc;
                                const float mn = fabsf(nyq);
                                nyq = mn > 0.0f ? nyq * (fmaxf(mn - p.v, 0.0f) / mn) : 0.0f;
                            }
                            if (inbuf) {
                                float2* o = reinterpret_cast<float2*>(p.out) + (size_t)b * n_bins * nF;
                                o[(size_t)bin * nF + f] = valid ? make_float2(re, im) : make_float2(0.f, 0.f);
                                if (dc) o[(size_t)(N / 2) * nF + f] = valid ? make_float2(nyq, 0.0f) : make_float2(0.f, 0.f);
                            }
                        } else {
                            mag[q] = sqrtf(re * re + im * im + p.mag_eps);
                            const float mnyq = sqrtf(nyq * nyq + p.mag_eps);
                            if (p.lin && inbuf) {
                                float* o = p.lin + ((size_t)b * nF + f) * n_bins;
                                o[bin] = valid ? mag[q] : 0.0f;
                                if (dc) o[N / 2] = valid ? mnyq : 0.0f;
                            }
                            // mel[m][frame] += basis[m][bin(k)] * mag[bin(k)][frame]: k = 0 is this register of lane half 0, k = 1 of half 1
#pragma unroll
                            for (int mt = 0; mt < 4; ++mt) {
                                if (mt < Mt) {
                                    const int m = mt * 32 + j;
                                    const float a = m < p.M ? p.melb[(size_t)m * n_bins + bin] : 0.0f;
                                    mel[mt][cb] = mfma32(a, mag[q], mel[mt][cb]);
                                }
                            }
                            if (rt == 0 && q == 0) {                        // the Nyquist bin: one more k-step, its second k slot empty
#pragma unroll
                                for (int mt = 0; mt < 4; ++mt) {
                                    if (mt < Mt) {
                                        const int m = mt * 32 + j;
                                        const float a = (m < p.M && h == 0) ? p.melb[(size_t)m * n_bins + N / 2] : 0.0f;
                                        mel[mt][cb] = mfma32(a, h == 0 ? mnyq : 0.0f, mel[mt][cb]);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    if constexpr (MODE == 1) {
        // partial mel tiles of the four waves -> LDS [frame][m] in the fixed order ((w0 + w1) + w2) + w3, then the log and the store
        const int MS = Mt * 32 + 1;
        for (int w = 0; w < 4; ++w) {
            __syncthreads();
            if (wave == w) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    if (mt < Mt) {
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int at = (cb * 32 + j) * MS + mt * 32 + frag_row(r, h);
                                lds[at] = w == 0 ? mel[mt][cb][r] : lds[at] + mel[mt][cb][r];
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int M = p.M;
        for (int idx = tid; idx < kStftNF * M; idx += kStftThreads) {
            const int fl = idx / M, m = idx - fl * M, f = f0 + fl;
            if (f >= nF) break;
            float o = 0.0f;
            if (f < nfb) {
                const double x = (double)fmaxf(lds[fl * MS + m], p.floor);
                o = (float)(p.log10 ? log10(x) : log(x));
            }
            p.out[((size_t)b * nF + f) * M + m] = o;
        }
    }
}

// Overlap-add as a gather (header comment, MODE 2).  frames [B][nF][N] windowed; wsq [N] = float32(w[n]^2), appended to the inverse basis.
struct IstftOlaParams {
    const float* frames;
    const float* wsq;
    const int* frame_counts;
    float* out;
    int nF, N, hop, trim, L_out;
};

__global__ void __launch_bounds__(256) k_istft_ola(IstftOlaParams p) {
    const int b = blockIdx.y;
    const long long t_out = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t_out >= p.L_out) return;
    const int nfb = p.frame_counts ? min(max(p.frame_counts[b], 0), p.nF) : p.nF;
    const long long t = t_out + p.trim;                                   // position in the untrimmed overlap-add buffer
    float sum = 0.0f, wss = 0.0f;
    if (nfb > 0 && t < (long long)p.N + (long long)p.hop * (nfb - 1) - p.trim) {
        long long flo = t - p.N + 1 <= 0 ? 0 : (t - p.N + p.hop) / p.hop;   // ceil((t - N + 1) / hop)
        long long fhi = t / p.hop;
        if (fhi > nfb - 1) fhi = nfb - 1;
        const float* fr = p.frames + (size_t)b * p.nF * p.N;
        for (long long f = flo; f <= fhi; ++f) {
            const int n = (int)(t - f * p.hop);
            sum += fr[(size_t)f * p.N + n];
            wss += p.wsq[n];
        }
        if (wss > FLT_MIN) sum /= wss;
    }
    p.out[(size_t)b * p.L_out + t_out] = sum;
}

// The packed bases, built on the device in float64 (exact angle reduction; cospi / sinpi of 2 m / N with m = (k n) mod N).
//   fwd: float4 index ((rt * (N / 8) + kq) * 64 + lane), element e = A[row rt * 32 + (lane & 31)][n = (kq * 4 + e) * 2 + (lane >> 5)]
//   inv: the same packing of the inverse basis, tile row 8 g + 4 hh + q holding sample rt * 32 + 16 hh + 4 g + q (see MODE 2), followed by
//        wsq[N] = float32(w[n]^2).
// w = the periodic Hann window of win_length samples centred in the frame (librosa.util.pad_center), zero outside.
__device__ __forceinline__ double stft_window(int n, int N, int win) {
    const int lp = (N - win) / 2;
    if (n < lp || n >= lp + win) return 0.0;
    return 0.5 - 0.5 * cospi(2.0 * (double)(n - lp) / (double)win);
}

__global__ void __launch_bounds__(256) k_stft_make_basis(float* fwd, float* inv, int N, int win) {
    const long long total = (long long)N * N;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total + N; idx += (long long)gridDim.x * 256) {
        if (idx >= total) {
            if (inv) { const double w = stft_window((int)(idx - total), N, win); inv[idx] = (float)(w * w); }
            continue;
        }
        const int e = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        const long long blk = idx >> 8;
        const int kq = (int)(blk % (N / 8)), rt = (int)(blk / (N / 8));
        const int tr = lane & 31, col = (kq * 4 + e) * 2 + (lane >> 5);
        if (fwd) {
            const int row = rt * 32 + tr, n = col;
            const int k = row == 1 ? N / 2 : (row >> 1);
            const int m = (int)(((long long)k * n) % N);
            const double w = stft_window(n, N, win);
            const double val = (row == 1 || !(row & 1)) ? w * cospi(2.0 * m / (double)N) : -w * sinpi(2.0 * m / (double)N);
            fwd[idx] = (float)val;
        }
        if (inv) {
            const int n = rt * 32 + 16 * ((tr >> 2) & 1) + 4 * (tr >> 3) + (tr & 3), c = col;
            const int k = c == 1 ? N / 2 : (c >> 1);
            const int m = (int)(((long long)k * n) % N);
            const double w = stft_window(n, N, win) / (double)N;
            double val;
            if (c == 0) val = w;
            else if (c == 1) val = w * cospi(2.0 * m / (double)N);
            else if (!(c & 1)) val = 2.0 * w * cospi(2.0 * m / (double)N);
            else val = -2.0 * w * sinpi(2.0 * m / (double)N);
            inv[idx] = (float)val;
        }
    }
}

}  // namespace dsd
