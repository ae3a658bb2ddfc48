/* dsv.h - C ABI of the HiFi-GAN / NSF-HiFi-GAN generator ops in libdsdenoise.so (MI355X, gfx950).
 *
 * the step AFTER the diffusion hot path - mel [B,80,T] (+ f0 [B,T]) -> waveform [B,1,T*hop].
 * The reference (MoonInTheRiver/DiffSinger) computes it with torch nn modules (modules/hifigan/hifigan.py:104-179,
 * modules/parallel_wavegan/models/source.py:7-137, :484-531, called from vocoders/hifigan.py:55-69) and has no FFI; these are
 * the operators its modules would bind.  Every entry point names the reference code it replaces (paths relative to the
 * reference root).  Conventions as in dsd.h: fp32 device pointers, `stream` a hipStream_t as void*, work is only ENQUEUED,
 * 0 on success / negative dsd_status otherwise with the message in dsd_last_error().
 *
 * Activation layout ("channel-major"): [B][C][LS], sample axis contiguous, LS = dsv_padded_samples(L) (L rounded up to a
 * multiple of 32); every op writes ZERO to the samples [L, LS) and expects that of its inputs.  Stateless: the caller owns
 * every buffer. */
#ifndef DSV_H
#define DSV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSV_ACT_NONE 0
#define DSV_ACT_TANH 1      /* torch.tanh after conv_post, modules/hifigan/hifigan.py:167-168 */

int32_t dsv_padded_samples(int32_t L);

/* Replaces the parameter storage of a Conv1d / ConvTranspose1d AFTER remove_weight_norm() (hifigan.py:171-179): a
 * convolution weight [rows][Ci][K] repacked into the MFMA A-operand fragment order dsv_conv1d streams (rows padded to 32,
 * Ci to 8, with zeros).  dsv_packed_floats = floats the packed buffer must hold (or -1).
 * For ConvTranspose1d(Ci, Co, k, stride u, padding (k-u)/2) the caller passes the polyphase form: rows = Co * u,
 * row co * u + r holds the taps that reach output phase r (see dsv_conv1d). */
int64_t dsv_packed_floats(int32_t rows, int32_t Ci, int32_t K);
int dsv_pack_weight(const float* w, int32_t rows, int32_t Ci, int32_t K, float* packed, void* stream);

/* [R][L] contiguous rows -> [R][LS] padded rows with a zero tail (the mel [B,80,T] entering conv_pre, hifigan.py:151). */
int dsv_pad_rows(const float* in, float* out, int64_t R, int32_t L, void* stream);

/* One convolution of the generator with its element-wise neighbours fused - Conv1d / ConvTranspose1d of
 * HifiGanGenerator.forward (hifigan.py:144-169), ResBlock1.forward (:54-61), ResBlock2.forward (:82-87):
 *     y[row][q] = sum_ci sum_k  W[row][ci][k] * leaky_relu(in[ci][q + k * dil - pad], pre_slope)      (zero outside [0, L_in))
 *     co = row / up, phase = row % up, n = q * up + phase                                              (up = 1: plain Conv1d)
 *     v = y + bias[co] ; v += residual[co][n] ; v = sum_in[co][n] + v ; v = v / divide ; v = act(v)  -> out[co][n]
 * in [B][Ci][LS(L_in)]; out / residual / sum_in [B][rows / up][LS(L_in * up)]; bias [rows / up]; residual, sum_in, bias may be
 * NULL; pre_slope 1 = no activation in front, divide 1 = none.  Taps must stay within +-48 samples (pad <= 48 and
 * (K-1) * dil - pad <= 48: kernel 11 at dilation 5 reaches 25 on the shipped generators, the official v3's kernel 7 at dilation 12
 * reaches 36; beyond +-28 a second instantiation of the kernel with a wider staged window runs).
 * Covers: `leaky_relu -> convs1[i]`, `leaky_relu -> convs2[i] -> + x` (residual), the last conv of resblock j adding into
 * the running `xs` (sum_in) and the last one also doing `/ num_kernels` (divide), `leaky_relu -> ups[i] (+ x_source)`
 * (up = stride, residual = the noise_convs output), conv_pre, and `leaky_relu(0.01) -> conv_post -> tanh`. */
int dsv_conv1d(const float* in, const float* wpacked, const float* bias, float* out, int32_t B, int32_t Ci, int32_t rows, int32_t K,
               int32_t pad, int32_t dil, int32_t L_in, int32_t up, float pre_slope, const float* residual, const float* sum_in,
               float divide, int32_t act, void* stream);

/* `ngroups` (1 .. 3) INDEPENDENT convolutions of the same shape (B, Ci, rows, L_in, up, pre_slope) in ONE launch (round 6) - the
 * convolutions of the parallel resblocks of a stage, level by level (hifigan.py:161-166: `resblocks[i * num_kernels + j](x)` for j = 0, 1, 2
 * read the same x and depend on nothing of each other until `xs +=`).  Convolution g is exactly dsv_conv1d(d[g].in, d[g].wpacked, ...,
 * d[g].act) - kernel size, padding, dilation, residual, running sum, divisor and activation are its own; the workgroups of d[0] are
 * dispatched first (pass the largest kernel first).  No output may be an operand of another convolution of the call.  On the 64-channel
 * stage of the shipped generator a convolution is one round of co-resident workgroups and a launch costs 15-19 us beyond its matrix time:
 * three convolutions per launch pay that once.  Same tiles, same chunk order as dsv_conv1d: bit-identical. */
typedef struct dsv_conv_desc {
    const float* in;
    const float* wpacked;
    const float* bias;
    float* out;
    const float* residual;
    const float* sum_in;
    int32_t K, pad, dil, act;
    float divide;
    int32_t reserved;
} dsv_conv_desc;
int dsv_conv1d_multi(int32_t ngroups, const dsv_conv_desc* d, int32_t B, int32_t Ci, int32_t rows, int32_t L_in, int32_t up, float pre_slope,
                     void* stream);

/* A/B switch of the measurement (round 6): the stride-2 transposed convolutions (up = 2, rows <= 32, taps within 4 samples) run on a lean build
 * of the same kernel - half the tile, LDS by the channel count, at most 128 registers: four and more workgroups per CU instead of two - the
 * same chunk order, the same bits; 0 = the standard build.  Process-wide, not thread-safe. */
int dsv_set_lean(int32_t on);

/* The same convolution (up = 1, 'same' padding pad = (K-1) * dil / 2, K odd) for the NARROW layers, Co <= 16 - the 16- and 8-channel
 * resblocks and conv_post of the shipped generator: F output samples are folded into the 32 MFMA rows so that no row multiplies
 * zeros.  dsv_fold_factor returns the F the library wants for such a layer (4: Co <= 8, 2: Co <= 16, 1: use dsv_conv1d; also 1
 * after dsv_set_fold(0) - the A/B switch of the measurement).  The caller packs, with
 * dsv_pack_weight(rows = Co * F, Ci, K + F - 1), the F shifted copies of the filter
 *     W'[co * F + e][ci][s] = w[co][ci][s - e]   (0 <= s - e < K, else 0)
 * and the kernel evaluates, with pos(c) = (c / dil) * F * dil + c % dil,
 *     out[co][pos(c) + e * dil] = sum_ci sum_s W'[co * F + e][ci][s] * leaky_relu(in[ci][pos(c) + s * dil - pad])   + the same fused tail
 * which is the convolution of dsv_conv1d sample for sample (every output sample is produced by exactly one (c, e)). */
int32_t dsv_fold_factor(int32_t Co, int32_t Ci, int32_t K, int32_t dil);
int dsv_set_fold(int32_t on);
int dsv_conv1d_folded(const float* in, const float* wpacked, const float* bias, float* out, int32_t B, int32_t Ci, int32_t Co, int32_t K,
                      int32_t F, int32_t dil, int32_t L, float pre_slope, const float* residual, const float* sum_in, float divide,
                      int32_t act, void* stream);

/* Whole ResBlock1 chains in ONE launch, activations resident in LDS (csrc/voc_chain.hpp) - `xs = sum_r resblock_r(x)` of
 * HifiGanGenerator.forward (hifigan.py:161-166) with ResBlock1.forward (:54-61) inside:
 *     for r < nres:  y = x ; for q < npairs:  xt = conv[r][q][0](leaky_relu(y)) ; xt = conv[r][q][1](leaky_relu(xt)) ; y = xt + y
 *     out = (sum_in + y_0 + y_1 + ...) / divide            (sum_in may be NULL: the running `xs` of resblocks that ran before this call)
 * for C = 8, 16 or 32 channels (C * F == 32 with the fold F = dsv_chain_fold(C) = 4, 2, 1 of dsv_conv1d_folded).  in, out, sum_in:
 * [B][C][LS(L)], in != out, sum_in != out (out carries the running sum over the call's resblocks while it runs).  convs: HOST array [nres][npairs][2] - the first convolution of a pair at dilation `dil`, the second at 1
 * ('same' padding, K odd); w_offset = float offset of its packed weight inside `wpacked` (each piece = dsv_pack_weight(rows = 32,
 * Ci = C, K + F - 1) of the F shifted copies W'[co * F + e][ci][s] = w[co][ci][s - e], pieces at multiples of 256 floats, the buffer
 * ending with the slack dsv_packed_floats includes), bias_offset = float offset of its bias [C] inside `bias`.  A workgroup owns N output
 * samples plus a halo of the chain's receptive field; dsv_chain_supported returns that N (0: the chain does not fit the staged tile -
 * kernel / dilation too wide, too many convolutions - run it convolution by convolution with dsv_conv1d / dsv_conv1d_folded).  The
 * summation order of every output sample is the one of those operators: the results are bit-identical to theirs. */
typedef struct dsv_chain_conv {
    int64_t w_offset;
    int32_t bias_offset;
    int32_t K;
    int32_t dil;
    int32_t reserved;
} dsv_chain_conv;
int32_t dsv_chain_fold(int32_t C);
int32_t dsv_chain_supported(int32_t C, int32_t nres, int32_t npairs, const dsv_chain_conv* convs);
int dsv_resblock_chain(const float* in, const float* wpacked, const float* bias, float* out, const float* sum_in, int32_t B, int32_t C,
                       int32_t L, int32_t nres, int32_t npairs, const dsv_chain_conv* convs, float pre_slope, float divide, void* stream);
/* The parallel resblocks of a stage as TWO launches instead of one per resblock (round 6).  A chain launch of W workgroups on S co-resident
 * slots (256 CUs x 2 or 3) takes ceil(W / S) rounds, not W / S (profiles/r6_27_voc_tail_probe.jsonl): three dependent launches pay three
 * partial last rounds.  dsv_resblock_chain_multi runs `ngroups` (1 .. 3) INDEPENDENT single-resblock chains in one grid - group g =
 * convs[g][npairs][2] over the whole input, its raw y_g (no sum, no division, NOT zeroed in [L, LS)) to outs[g] (a HOST array of device
 * pointers, all different, none the input); the workgroups of group 0 are dispatched first: pass the longest chain first, so that the
 * short workgroups of a later group fill its last round.  dsv_resblock_chain_sum then runs ONE more resblock and forms the stage's result
 * in the order of `xs += resblock(x)` (hifigan.py:161-166): out = ((sum_in + y) + sum_in2) / divide - this resblock first or second of
 * three - or, own_last != 0, ((sum_in + sum_in2) + y) / divide; zero in [L, LS).  No workgroup waits for another; an ordinary kernel
 * boundary orders the two launches.  Same sums in the same order as dsv_resblock_chain: bit-identical.  Which resblock to leave for the
 * second launch is the caller's choice (diffsinger_amd/vocoder.py _merge_plan: the split with the fewest modelled rounds). */
int dsv_resblock_chain_multi(const float* in, const float* wpacked, const float* bias, float* const* outs, int32_t B, int32_t C, int32_t L,
                             int32_t ngroups, int32_t npairs, const dsv_chain_conv* convs, float pre_slope, void* stream);
int dsv_resblock_chain_sum(const float* in, const float* wpacked, const float* bias, float* out, const float* sum_in, const float* sum_in2,
                           int32_t own_last, int32_t B, int32_t C, int32_t L, int32_t npairs, const dsv_chain_conv* convs, float pre_slope,
                           float divide, void* stream);
/* A/B switch of the measurement: which instantiation of the chain kernel C = 8 / 16 / 32 channels run on - `nb` column blocks of 32 per wave
 * (a workgroup's window is 128 * nb * F samples; 2 or 4) and ONE LDS tile rewritten in place (in_place = 1: half the LDS, twice the workgroups
 * per CU or twice the window) or the two tiles of rounds 3-5 (in_place = 0).  Every variant evaluates the same sums in the same order: the
 * results do not depend on it.  dsv_chain_supported answers for the variant in force.  Process-wide, not thread-safe (a test / bench switch). */
int dsv_set_chain_variant(int32_t C, int32_t nb, int32_t in_place);
/* Measurement hook: DEVICE buffer of 18 * 4 * 4 uint64 (or NULL to switch it off) - the following dsv_resblock_chain launches record the
 * shader clock of ONE workgroup (the middle tile of utterance 0) per convolution n and wave w at [n][w][0..3] = {convolution start,
 * contraction done, epilogue done, barrier passed}. */
int dsv_debug_chain_timeline(uint64_t* device_stamps);

/* noise_convs[i] (hifigan.py:124-130, :158-160): the strided Conv1d(1 -> C, kernel K, stride, padding) over the harmonic
 * source.  har [B][LS(L_har)], w [C][K] (the torch weight [C][1][K]), bias [C] or NULL, out [B][C][LS(L_out)];
 * L_out must equal (L_har + 2 * pad - K) / stride + 1. */
int dsv_noise_conv(const float* har, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t K, int32_t stride,
                   int32_t pad, int32_t L_har, int32_t L_out, void* stream);

/* torch.nn.Upsample(scale_factor = up) of f0 + SourceModuleHnNSF.forward (source.py:518-531) = SineGen.forward (:101-137,
 * _f02sine :45-77, flag_for_pulse False) -> Linear(H, 1) -> tanh.  The module's random draws are INPUTS (the caller draws them
 * with whatever generator it must match): rand_ini [B][H] uniform [0,1) (column 0 is ignored), noise [B][L][H] standard
 * normal, L = T * up.  f0 [B][T] Hz (<= voiced_threshold = unvoiced), lin_w [H], lin_b [1]; sines_ws: workspace of
 * B * H * L floats; har [B][LS(L)] = the merged harmonic source (the module's `noise` output is never used by the generator).
 * Both cumulative sums over the sample axis accumulate in fp64, as aten's CPU cumsum does for float tensors. */
int dsv_sine_source(const float* f0, const float* rand_ini, const float* noise, const float* lin_w, const float* lin_b, float* sines_ws,
                    float* har, int32_t B, int32_t T, int32_t up, int32_t H, float sample_rate, float sine_amp, float noise_std,
                    float voiced_threshold, void* stream);

/* ParallelWaveGAN generator (vocoders/pwg.py; modules/parallel_wavegan/models/parallel_wavegan.py:21-177) - residual_channels 64, gate_channels
 * 128, skip_channels 64, kernel_size 3 (the configuration the reference ships and trains); activations [B][C][LS(L)] like the HiFi-GAN ops.
 * dsv_pwg_first: first_conv, Conv1d1x1(1, C) on the noise z [B][LS]: out[b][c][t] = w[c] z[b][t] + bias[c].
 * dsv_pwg_upsample: one stage of UpsampleNetwork (layers/upsample.py:96-117) on `rows` = B * C rows: nearest-neighbour stretch by `scale`, then the
 *   (2 scale + 1)-tap filter the Conv2d(1, 1, (1, 2 scale + 1), padding (0, scale), bias=False) shares between all rows.
 * dsv_pwg_layer: one ResidualBlock (layers/residual_block.py:96-129):
 *     a = conv(x; kernel 3, dilation dil, 'same') + b1 + conv1x1_aux(c);  z = tanh(a[0:64]) * sigmoid(a[64:128])
 *     x_out = (conv1x1_out(z) + x) * sqrt(0.5);   skip = (first ? 0 : skip) + conv1x1_skip(z)
 *   w1_packed = dsv_pack_weight of the [128][3 * 64 + n_aux][1] matrix whose columns are tap * 64 + ci (tap 0 reads t - dil) followed by the aux
 *   channels; w2_packed = dsv_pack_weight of [128][64][1], rows 0..63 conv1x1_out, 64..127 conv1x1_skip; b1 [128] / b2 [128] may be NULL.
 *   Any dilation (the generator's run to 512 samples); x_out must not alias x. */
int dsv_pwg_first(const float* z, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t L, void* stream);
int dsv_pwg_upsample(const float* in, const float* filter, float* out, int64_t rows, int32_t L_in, int32_t scale, void* stream);
int dsv_pwg_layer(const float* x, const float* c, const float* w1_packed, const float* b1, const float* w2_packed, const float* b2, float* x_out,
                  float* skip, int32_t B, int32_t L, int32_t n_aux, int32_t dil, int32_t first, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * STFT: framed real DFT, its inverse with overlap-add, the spectral-subtraction post-filter and the log-mel analysis (csrc/voc_stft.hpp) -
 * the other half of the vocoder interface (vocoders/base_vocoder.py:22-39: spec2wav AND wav2spec).  Waveforms are plain [B][L] rows here
 * (no LS padding).  The DFT is a matrix product on the fp32 MFMA against a precomputed basis with the window folded in; every sum runs in a
 * fixed order (two calls are bitwise equal), nothing allocates or synchronises.
 *
 * Supported: n_fft in {256, 512, 1024, 2048}, 1 <= win_length <= n_fft (periodic Hann window centred in the frame, zero outside - scipy's
 * get_window('hann', win_length) through librosa.util.pad_center), 1 <= hop <= n_fft, B <= 65535, L <= 2^30.  Everything else is refused with
 * DSD_ERR_INVALID before any launch.
 *
 * Bases: dsv_stft_basis_floats(n_fft, which) floats each (-1: unsupported n_fft); dsv_stft_make_basis fills either or both ON THE DEVICE in
 * float64 (angles reduced exactly, each entry the float32 rounding of the float64 value) - one launch, once per (n_fft, win_length); call it
 * outside a graph capture and keep the buffers.  DSV_STFT_BASIS_FWD carries the analysis window; DSV_STFT_BASIS_INV the synthesis window,
 * 1 / n_fft, the factor 2 of the interior bins, and behind them float32(w[n]^2) for the window sum-of-squares.
 *
 * Framing: pad_l / pad_r samples of padding per side applied by index arithmetic (DSV_STFT_PAD_CONSTANT: zeros, librosa.stft(pad_mode=
 * 'constant'), data_gen/tts/data_gen_utils.py:123-124; DSV_STFT_PAD_REFLECT: torch's 'reflect', modules/hifigan/mel_utils.py:66-71, pads < L);
 * "center" is pad_l = pad_r = n_fft / 2.  n_frames = dsv_stft_frames(L, ...) = 1 + (L + pad_l + pad_r - n_fft) / hop (-1: not one frame).
 * `lengths` (device int32 [B], or NULL): valid samples per row; a row then has 1 + (len + pad_l + pad_r - n_fft) / hop valid frames (0 when
 * that is not one frame; padding reflects about the row's own end), written to frames_out [B] (device, or NULL).  A length outside [0, L] is
 * clamped to it.  The reflect-padding condition pads < L is checked against L, not against lengths[b]: a row NO LONGER THAN ITS PADDING is
 * padded by a SINGLE reflection about its own first / last sample, and by 0 where that reflection leaves the row (torch refuses such a row;
 * a row of one sample is that sample between zeros).  FRAMES AT OR BEYOND A ROW'S VALID COUNT ARE WRITTEN AS EXACTLY 0 by dsv_stft and
 * dsv_logmel - the library's padding value for mels. */
#define DSV_STFT_BASIS_FWD 0
#define DSV_STFT_BASIS_INV 1
#define DSV_STFT_PAD_CONSTANT 0
#define DSV_STFT_PAD_REFLECT 1
int64_t dsv_stft_basis_floats(int32_t n_fft, int32_t which);
int dsv_stft_make_basis(int32_t n_fft, int32_t win_length, float* fwd, float* inv, void* stream);
int64_t dsv_stft_frames(int64_t L, int32_t n_fft, int32_t hop, int32_t pad_l, int32_t pad_r);

/* librosa.stft / torch.stft (vocoders/vocoder_utils.py:10; modules/hifigan/mel_utils.py:70-71 with complex=True): wav [B][L] ->
 * spec [B][n_fft / 2 + 1][n_frames][2], (re, im) interleaved - the memory of a complex64 tensor [B][n_bins][n_frames], torch.stft's layout.
 * subtract != 0 fuses the spectral subtraction of vocoders/vocoder_utils.py:11-13, np.clip(|S| - v, 0) * exp(i angle(S)) up to rounding:
 * S' = S * max(|S| - v, 0) / |S| (0 where |S| = 0); the unfiltered spectrum is never written. */
int dsv_stft(const float* wav, const int32_t* lengths, const float* fwd_basis, float* spec, int32_t* frames_out, int32_t B, int32_t L,
             int32_t n_fft, int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode, int32_t subtract, float v, void* stream);

/* librosa.istft (vocoders/vocoder_utils.py:14) as diffsinger_amd.vocoder.denoise restates it: inverse real DFT of every frame (the imaginary
 * parts of bin 0 and bin n_fft / 2 are ignored, as irfft does) times the synthesis window, overlap-added, divided by the window
 * sum-of-squares where that exceeds FLT_MIN, trimmed by n_fft / 2 per side when center != 0.  Two launches: the windowed frames
 * [B][n_frames][n_fft] go through `workspace` (dsv_istft_workspace_floats floats), then every output sample GATHERS its contributing frames
 * in ascending frame order (the order of the host loop) - a fused form would need 64 + 2 (n_fft / hop - 1) frames of n_fft floats in LDS,
 * 280 KiB at 1024 / 256.  wav [B][L_out]: L_out is the caller's row length, dsv_istft_samples(n_frames, ...) = n_fft + hop (n_frames - 1)
 * [- 2 (n_fft / 2)] samples of it are signal (per row: by frame_counts [B], device int32 or NULL), the rest is written 0. */
int64_t dsv_istft_samples(int64_t n_frames, int32_t n_fft, int32_t hop, int32_t center);
int64_t dsv_istft_workspace_floats(int32_t B, int64_t n_frames, int32_t n_fft);
int dsv_istft(const float* spec, const int32_t* frame_counts, const float* inv_basis, float* workspace, float* wav, int32_t B,
              int32_t n_frames, int32_t L_out, int32_t n_fft, int32_t hop, int32_t center, void* stream);

/* Log-mel analysis in one launch - process_utterance (data_gen/tts/data_gen_utils.py:122-134, behind vocoders/pwg.py:105-122 wav2spec) and
 * mel_spectrogram (modules/hifigan/mel_utils.py:59-76):
 *     x = clamp ? clip(wav, -1, 1) : wav;  S = stft(x);  mag = sqrt(re^2 + im^2 + mag_eps);  mel = mel_basis [M][n_bins] . mag
 *     out[b][frame][m] = log(max(mel, floor))       natural (log10 = 0) or base 10 (log10 != 0), evaluated in float64 and rounded once
 * mel_basis is DATA of the caller (M <= 128, row-major; librosa.filters.mel(...) or diffsinger_amd.stft.mel_filterbank); out
 * [B][n_frames][M], the [T, 80] layout of the library's mels; linear (or NULL) [B][n_frames][n_bins] receives mag.
 *   pwg:     pad_l = pad_r = n_fft / 2 constant, clamp 0, mag_eps 0, floor eps (wav2spec_eps), log10 1
 *   hifigan: pad_l = pad_r = (n_fft - hop) / 2 reflect, clamp 1, mag_eps 1e-9, floor 1e-5, log10 0 */
int dsv_logmel(const float* wav, const int32_t* lengths, const float* fwd_basis, const float* mel_basis, float* out, float* linear,
               int32_t* frames_out, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode,
               int32_t clamp, int32_t M, float mag_eps, float floor, int32_t log10, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * STFT loss: the multi-resolution STFT criterion of the vocoder trainers (modules/parallel_wavegan/losses/stft_loss.py, configured by
 * configs/tts/pwg.yaml:77-82) - the transpose of dsv_stft and the spectral loss over two spectra, forward and backward
 * (csrc/voc_stft_loss.hpp).  Fixed summation order, no atomics (two calls are bitwise equal), nothing allocates or synchronises, every
 * scalar the backward needs is read from device memory: the whole forward and backward records into one graph.
 *
 * Adjoint STFT - the vector-Jacobian product of dsv_stft (no lengths, no subtraction): grad_spec [B][n_fft / 2 + 1][n_frames][2], the
 * cotangent in the spectrum's own layout, -> grad_wav [B][L].  frame_grad[f][n] = sum_rows A[row][n] G[row][f] is the product dsv_istft
 * runs (the same kernel) against a third basis, DSV_STFT_BASIS_ADJ: the forward basis transposed - the ANALYSIS window, no 1 / n_fft, no
 * factor 2 on the interior bins; the imaginary cotangents of bin 0 and bin n_fft / 2 are ignored (the forward writes 0 there whatever the
 * signal).  dsv_stft_basis_floats(n_fft, DSV_STFT_BASIS_ADJ) floats, filled by dsv_stft_make_adjoint_basis (on the device in float64,
 * once per (n_fft, win_length), outside a capture).  The frame gradients go through `workspace` (dsv_stft_adjoint_workspace_floats
 * floats); then every sample of grad_wav GATHERS the values of its position of the padded signal in ascending frame order - no division
 * by a window sum.  Padding folds back by index arithmetic: DSV_STFT_PAD_CONSTANT drops what fell on the padding, DSV_STFT_PAD_REFLECT
 * adds to a sample the sums of the positions that mirrored it (left mirror, then right; a short row can have both).  L, n_fft, hop, pad_l,
 * pad_r, pad_mode are the forward call's and are refused as there. */
#define DSV_STFT_BASIS_ADJ 2
int dsv_stft_make_adjoint_basis(int32_t n_fft, int32_t win_length, float* adj, void* stream);
int64_t dsv_stft_adjoint_workspace_floats(int32_t B, int64_t n_frames, int32_t n_fft);
int dsv_stft_adjoint(const float* grad_spec, const float* adj_basis, float* workspace, float* grad_wav, int32_t B, int32_t L, int32_t n_fft,
                     int32_t hop, int32_t pad_l, int32_t pad_r, int32_t pad_mode, void* stream);

/* Spectral loss over two spectra X (the prediction) and Y (the recording), n complex elements each ((re, im) interleaved, any layout as
 * long as both share it):  P = re^2 + im^2,  m = sqrt(max(P, 1e-7))  (stft_loss.py:26-31),
 *     out[0] = sc  = ||ym - xm||_F / ||ym||_F  (:52)          out[1] = mag = mean |ln ym - ln xm|  (:73)
 * One pass over X and Y with float64 sums per thread and a fixed-order tree per workgroup, partials to `workspace`
 * (dsv_spectral_loss_workspace_floats(n) floats, 8-byte aligned; -1: n outside [1, 2^40]), one more launch adds them in index order and leaves
 * S1 = ||ym - xm||_F and S2 = ||ym||_F there for the backward.  Backward (same X, Y, workspace; grad_out [2] = (g_sc, g_mag) ON THE DEVICE):
 *     G = (re, im) * [ -g_sc (ym - xm) / (xm S1 S2) - g_mag sign(ln ym - ln xm) / (n P) ]     where P > 1e-7;  exactly 0 where the clamp is
 * active.  sign(0) = 0 and a zero difference contributes 0 (X = Y gives G = 0).  The gradient is with respect to X only. */
int64_t dsv_spectral_loss_workspace_floats(int64_t n);
int dsv_spectral_loss(const float* X, const float* Y, float* workspace, float* out, int64_t n, void* stream);
int dsv_spectral_loss_backward(const float* X, const float* Y, const float* workspace, const float* grad_out, float* G, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Mel loss: the log-mel analysis of modules/hifigan/mel_utils.py:45-76 as a DIFFERENTIABLE chain - the generator's dominant objective
 * (configs/tts/hifigan.yaml lambda_mel: the L1 distance of two log-mels) - csrc/voc_mel.hpp.  dsv_logmel above is the fused analysis and
 * has no gradient; here the chain is cut at the spectrum:  dsv_mel_spectrum -> dsv_mel_head,  and back  dsv_mel_head_backward ->
 * dsv_stft_adjoint -> dsv_mel_clamp_backward.  The L1 mean over the cells is dsf_l1_mean / dsf_l1_mean_bwd (include/dsf.h).  No atomics,
 * every sum in a fixed order (two calls are bitwise equal); nothing allocates or synchronises: forward and backward record into one graph.
 * Refused with DSD_ERR_INVALID before any launch: null pointers, n_fft not in {256, 512, 1024, 2048}, M outside [1, 128], T < 1 (or > 2^30),
 * B outside [1, 65535], mag_eps < 0, floor <= 0 or either not finite, an output that overlaps an input, a spectrum not aligned to 8 bytes.
 *
 * dsv_mel_spectrum: dsv_stft's launch (the same kernel, the same bits) with the waveform clamp of dsv_logmel exposed: clamp != 0 reads
 *   clip(wav, -1, 1).  No lengths, no subtraction.  spec [B][n_fft / 2 + 1][n_frames][2].
 * dsv_mel_head: spec [B][n_bins][T][2], n_bins = n_fft / 2 + 1, mel_basis [M][n_bins] (data of the caller) ->
 *       mag = sqrt(re^2 + im^2 + mag_eps);   mel[b][f][m] = sum_k mel_basis[m][k] mag[k][f];   out[b][f][m] = log(max(mel, floor))
 *   natural (log10 = 0) or base 10, evaluated in float64 and rounded once.  out and mel [B][T][M] are BOTH written (the backward reads mel).  All
 *   bins are treated alike: whatever imaginary part the caller stored at bins 0 and n_fft / 2 counts.  fp32 MFMA, one launch.
 * dsv_mel_head_backward: the vector-Jacobian product for a cotangent grad_out [B][T][M], with the forward's spec, mel_basis and mel:
 *       gm = grad_out / mel [/ ln 10] where mel >= floor, else exactly 0  (torch.clamp(min=)'s rule: the gradient passes at equality)
 *       G[b][k][f] = (re, im) / mag * sum_m mel_basis[m][k] gm[f][m]      exactly 0 where mag == 0 (only possible with mag_eps = 0)
 *   G [B][n_bins][T][2], the layout dsv_stft_adjoint takes.  fp32 MFMA, one launch.
 * dsv_mel_clamp_backward: dx_out[i] = dx_in[i] where -1 <= x[i] <= 1, else 0, over n floats (a NaN x gives 0); dx_out may BE dx_in. */
int dsv_mel_spectrum(const float* wav, const float* fwd_basis, float* spec, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t pad_l,
                     int32_t pad_r, int32_t pad_mode, int32_t clamp, void* stream);
int dsv_mel_head(const float* spec, const float* mel_basis, float* out, float* mel, int32_t B, int32_t T, int32_t n_fft, int32_t M, float mag_eps,
                 float floor, int32_t log10, void* stream);
int dsv_mel_head_backward(const float* spec, const float* mel_basis, const float* grad_out, const float* mel, float* G, int32_t B, int32_t T,
                          int32_t n_fft, int32_t M, float mag_eps, float floor, int32_t log10, void* stream);
int dsv_mel_clamp_backward(const float* x, const float* dx_in, float* dx_out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * PWG discriminator: ParallelWaveGANDiscriminator (modules/parallel_wavegan/models/parallel_wavegan.py:207-300; configs/tts/pwg.yaml
 * discriminator_params: 10 layers, 64 channels, kernel 3, LeakyReLU(0.2)) forward AND backward, and the LSGAN criterion
 * (modules/hifigan/hifigan.py:337-365) - csrc/pwg_disc.hpp.  Activations [B][64][LS(T)] channel-major, waveform-like rows [B][LS(T)]; every call
 * leaves [T, LS) of its outputs at zero.  Exact fp32 (MFMA with fp32 accumulation), no atomics, fixed summation order (two calls are bitwise
 * equal); nothing allocates or synchronises, every scalar is read from device memory: forward, loss and backward record into one graph.
 * B in [1, 65535], T in [1, 2^30], 0 < slope < 1, 1 <= dil <= 8; anything else is refused with DSD_ERR_INVALID before any launch.
 *
 * dsv_pwgd_tile(): samples per workgroup of dsv_pwgd_layer.  dsv_pwgd_wgrad_split(): samples per workgroup of dsv_pwgd_wgrad; its workspace is
 * dsv_pwgd_wgrad_workspace_floats(B, T) = B * ceil(T / split) * (64 * 64 * 3 + 64) floats (-1: bad shape).
 *
 * dsv_pwgd_layer: one 64 -> 64 layer (kernel 3, dilation dil, 'same' zero padding), one launch.
 *   backward == 0:  out = leaky_relu(W in + bias, slope);  w_packed = dsv_pack_weight of the [64][192][1] matrix with columns tap * 64 + ci
 *                   (tap 0 reads t - dil); bias [64] or NULL; saved must be NULL.
 *   backward != 0:  out = (W^T * in) m - `in` the gradient with respect to this layer's pre-activation, out the gradient with respect to the
 *                   pre-activation of the layer below; m = 1 where saved (that layer's POST-activation, [B][64][LS]) > 0, else slope (a saved
 *                   value of exactly 0 takes the slope, as autograd does for an in-place LeakyReLU); saved NULL: no mask.  w_packed =
 *                   dsv_pack_weight of [64][192][1] with row ci, column tap * 64 + co = W[co][ci][2 - tap]; bias must be NULL.
 *   out must not alias in.  Several layers' matrices may be packed by ONE dsv_pack_weight call of [n * 64][192][1]: layer i's stream starts
 *   2 * i * 24 * 256 floats into the buffer.
 * dsv_pwgd_wgrad: dw[co][ci][k] = sum_b sum_t g[b][co][t] a_prev[b][ci][t + (k - 1) dil] (torch layout [64][64][3]), db[co] = sum_b sum_t
 *   g[b][co][t] (db NULL: not written).  Two launches: split partials on the MFMA, then the splits added in index order in float64.
 * dsv_pwgd_first: x [B][LS] -> out [B][64][LS] = leaky_relu(conv(x; w [64][1][3], dilation 1) + bias).  dsv_pwgd_first_backward: from g0 (the
 *   gradient with respect to the first layer's pre-activation) dw [64][3], db [64] (or NULL), and dx [B][LS] - only when dx is not NULL (one
 *   launch less).  dsv_pwgd_last: a [B][64][LS] -> out [B][LS] = conv(a; w [1][64][3], dilation 1) + bias[0], no activation.
 *   dsv_pwgd_last_backward: from gp [B][LS] (zero in [T, LS)) dw [64][3], db [1] (or NULL) and ga = (w^T * gp) m(a) [B][64][LS].  The parameter
 *   gradients of both use a workspace of dsv_pwgd_edge_workspace_floats(B, T) floats and sum in float64 in a fixed order.
 * LSGAN: out[0] = mean((d[i] - target)^2) over n floats (float64 partial sums in `workspace`, dsv_pwgd_lsgan_workspace_floats(n) floats, 8-byte
 *   aligned; -1: n outside [1, 2^40]); backward G[i] = 2 (d[i] - target) / n * grad_out[0], grad_out ON THE DEVICE. */
int32_t dsv_pwgd_tile(void);
int32_t dsv_pwgd_wgrad_split(void);
int64_t dsv_pwgd_wgrad_workspace_floats(int32_t B, int32_t T);
int64_t dsv_pwgd_edge_workspace_floats(int32_t B, int32_t T);
int dsv_pwgd_layer(const float* in, const float* w_packed, const float* bias, const float* saved, float* out, int32_t B, int32_t T, int32_t dil,
                   float slope, int32_t backward, void* stream);
int dsv_pwgd_wgrad(const float* g, const float* a_prev, float* workspace, float* dw, float* db, int32_t B, int32_t T, int32_t dil, void* stream);
int dsv_pwgd_first(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t T, float slope, void* stream);
int dsv_pwgd_first_backward(const float* g0, const float* x, const float* w, float* workspace, float* dw, float* db, float* dx, int32_t B,
                            int32_t T, void* stream);
int dsv_pwgd_last(const float* a, const float* w, const float* bias, float* out, int32_t B, int32_t T, void* stream);
int dsv_pwgd_last_backward(const float* gp, const float* a, const float* w, float* workspace, float* dw, float* db, float* ga, int32_t B, int32_t T,
                           float slope, void* stream);
int64_t dsv_pwgd_lsgan_workspace_floats(int64_t n);
int dsv_pwgd_lsgan(const float* d, float target, float* workspace, float* out, int64_t n, void* stream);
int dsv_pwgd_lsgan_backward(const float* d, float target, const float* grad_out, float* G, int64_t n, void* stream);

/* PWG generator training: the training forward of a gated residual block and the backward of every piece of ParallelWaveGANGenerator
 * (modules/parallel_wavegan/models/parallel_wavegan.py:21-177, layers/residual_block.py:96-129, layers/upsample.py:63-183) - csrc/pwg_train.hpp.
 * Activations [B][C][LS(L)] channel-major; every call leaves [L, LS) of its outputs at zero.  fp32 MFMA contractions, no atomics, fixed
 * summation order (two calls are bitwise equal); nothing allocates or synchronises.  B in [1, 65535], L in [1, 2^30], n_aux a multiple of 8 in
 * [0, 128], dil >= 1; anything else is refused with DSD_ERR_INVALID before any launch.  s = sqrt(0.5).
 *
 * dsv_pwgt_layer: dsv_pwg_layer (same arguments, bitwise the same x_out and skip) that also stores the gate pre-activations
 *   a_out [B][128][LS] = W_conv * [x(t - d); x(t); x(t + d)] + b_conv + W_aux c (rows 0..63 the tanh half, 64..127 the sigmoid half).
 * dsv_pwgt_gate_backward: dz = W_skip^T d_skip + W_out^T (s dx_next), da[0:64] = dz sigmoid(g) (1 - tanh(a)^2), da[64:128] = dz tanh(a) sigmoid(g)
 *   (1 - sigmoid(g)) with tanh / sigmoid recomputed from `a` by the forward's formulas.  w2t_packed = dsv_pack_weight of [64][128][1]: row ci,
 *   columns 0..63 = W_skip[co][ci], 64..127 = W_out[co][ci].  dx_next NULL (the last block: its residual output is never read): the out half
 *   is not multiplied.  Several blocks' matrices may be packed by ONE dsv_pack_weight call of [n * 64][128][1]: block i's stream starts
 *   2 * i * 16 * 256 floats into the buffer.
 * dsv_pwgt_conv_backward: dx = s dx_next + sum_tap W_conv[:, :, tap]^T da(t - (tap - 1) dil) (zero outside [0, L)); dx_next may be NULL;
 *   w1t_packed = dsv_pack_weight of [64][384][1]: row ci, column tap * 128 + co = W_conv[co][ci][tap] (block i at 2 * i * 48 * 256 floats).
 *   n_aux > 0: dc [B][n_aux][LS] (+)= W_aux^T da - written when first != 0, added to otherwise; wauxt_packed = dsv_pack_weight of
 *   [R][128][1], R = n_aux rounded up to 32: row r, column co = W_aux[co][r], rows >= n_aux zero (block i at (R / 32) * i * 16 * 256 floats).
 *   dx must not alias dx_next.
 * dsv_pwgt_wgrad_*: gradients of the 128-row matrices, out = dW [128][N] followed by db [128]; split partials on the MFMA into `workspace`
 *   (dsv_pwgt_wgrad_workspace_floats(B, L, N) = B * ceil(L / dsv_pwgt_wgrad_split()) * (128 N + 128) floats; -1: bad shape), then the splits added
 *   in index order in float64.
 *     _conv: N = 192 + n_aux, dW = sum_t da(t) [x(t - dil); x(t); x(t + dil); c(t)]^T (columns tap * 64 + ci, then the aux channels; the columns
 *            of a tap that lies outside the signal for every t are exact zeros), db = sum_t da.
 *     _out:  N = 64, rows 0..63 = sum_t s dx_next(t) z(t)^T (zeros when dx_next is NULL), rows 64..127 = sum_t d_skip(t) z(t)^T, z = tanh(a[0:64])
 *            sigmoid(a[64:128]) recomputed from `a`; db alike.
 *     _relu: N = 64, rows 0..63 = sum_t g(t) relu(saved(t))^T with g, saved [B][64][LS] (last_conv_layers[1]); rows 64..127 zero.
 * dsv_pwgt_rowdot: out[2 c] = sum_b sum_t P q(Q), out[2 c + 1] = sum_b sum_t P for c < C; P is [B][C][LS] when p_per_channel else [B][LS]
 *   shared by every channel, Q alike; q = relu when relu_q.  float64 sums in a fixed order.  (first_conv: P = dx0, Q = the noise;
 *   last_conv_layers[3]: P = the output gradient, Q = its saved input.)
 * dsv_pwgt_last_dgrad: out[b][c][t] = w[c] g[b][t] where saved[b][c][t] > 0, else 0 (g [B][LS], saved / out [B][C][LS]).
 * dsv_pwgt_relu_mask: out = scale * g where saved > 0, else 0, on `rows` rows of LS(L) samples.
 * dsv_pwgt_upsample_backward: one stage of dsv_pwg_upsample.  g [rows][LS(L_in * scale)], in [rows][LS(L_in)], filter [2 scale + 1] ->
 *   dw [2 scale + 1] (float64 partials per row in `workspace`, dsv_pwgt_upsample_workspace_floats(rows, scale) floats, 8-byte aligned, added in
 *   row order) and, when din is not NULL, din [rows][LS(L_in)].
 * dsv_pwgt_convin_wgrad: dw[co][ci][k] = sum_b sum_t g[b][co][t] c[b][ci][t + k], g [B][C][LS(L_out)], c [B][C][LS(L_out + K - 1)] (conv_in: no
 *   padding); float64, fixed order. */
int32_t dsv_pwgt_wgrad_split(void);
int64_t dsv_pwgt_wgrad_workspace_floats(int32_t B, int32_t L, int32_t n_cols);
int64_t dsv_pwgt_upsample_workspace_floats(int64_t rows, int32_t scale);
int dsv_pwgt_layer(const float* x, const float* c, const float* w1_packed, const float* b1, const float* w2_packed, const float* b2, float* x_out,
                   float* skip, float* a_out, int32_t B, int32_t L, int32_t n_aux, int32_t dil, int32_t first, void* stream);
int dsv_pwgt_gate_backward(const float* dx_next, const float* d_skip, const float* a, const float* w2t_packed, float* da, int32_t B, int32_t L,
                           void* stream);
int dsv_pwgt_conv_backward(const float* da, const float* dx_next, const float* w1t_packed, const float* wauxt_packed, float* dx, float* dc, int32_t B,
                           int32_t L, int32_t n_aux, int32_t dil, int32_t first, void* stream);
int dsv_pwgt_wgrad_conv(const float* da, const float* x, const float* c, float* workspace, float* out, int32_t B, int32_t L, int32_t n_aux,
                        int32_t dil, void* stream);
int dsv_pwgt_wgrad_out(const float* dx_next, const float* d_skip, const float* a, float* workspace, float* out, int32_t B, int32_t L, void* stream);
int dsv_pwgt_wgrad_relu(const float* g, const float* saved, float* workspace, float* out, int32_t B, int32_t L, void* stream);
int dsv_pwgt_rowdot(const float* P, const float* Q, float* out, int32_t B, int32_t C, int32_t L, int32_t p_per_channel, int32_t q_per_channel,
                    int32_t relu_q, void* stream);
int dsv_pwgt_last_dgrad(const float* g, const float* saved, const float* w, float* out, int32_t B, int32_t C, int32_t L, void* stream);
int dsv_pwgt_relu_mask(const float* g, const float* saved, float* out, float scale, int64_t rows, int32_t L, void* stream);
int dsv_pwgt_upsample_backward(const float* g, const float* in, const float* filter, float* workspace, float* din, float* dw, int64_t rows,
                               int32_t L_in, int32_t scale, void* stream);
int dsv_pwgt_convin_wgrad(const float* g, const float* c, float* dw, int32_t B, int32_t C, int32_t K, int32_t L_out, void* stream);

/* HiFi-GAN generator training: the backward of every piece of HifiGanGenerator.forward (modules/hifigan/hifigan.py:30-92, :104-169,
 * modules/parallel_wavegan/models/source.py:518-531) - csrc/hifigan_train.hpp.  The training forward is the one-launch-per-convolution path above
 * (dsv_conv1d / dsv_conv1d_folded): every convolution's input is a tensor in memory, and the leaky ReLU in front of it is applied while staging.
 * Activations [B][C][LS(L)] channel-major; every call leaves [L, LS) of its outputs at zero.  No atomics, fixed summation order (two calls are
 * bitwise equal); nothing allocates or synchronises; everything is enqueued on `stream`.  B in [1, 65535], L (times `up`) in [1, 2^30], channels
 * in [1, 1024], taps within +-48 samples; anything else is refused with DSD_ERR_INVALID before any launch.  m(x) = x > 0 ? 1 : slope.
 *
 * dsv_hgt_act_floats(B, C, L) = B * C * LS(L): the length of an activation; dsv_hgt_wgrad_workspace_floats(B, L, Co, Ci, K, up) =
 *   B * ceil(L / dsv_hgt_wgrad_split()) * (Co * up) * (Ci * K): the workspace of dsv_hgt_conv_wgrad (-1: bad shape).
 * dsv_hgt_conv_dgrad: dx[b][i][t] = (m(x_saved) * sum_o sum_k w[o][i][k] g[b][o][t - k dil + pad] + residual + sum_in) / divide, g [B][Cg][LS],
 *   x_saved / residual / sum_in / dx [B][C][LS] (x_saved NULL: m = 1; residual / sum_in NULL: absent).  wt_packed = dsv_pack_weight of the flipped,
 *   transposed filter W'[i][o][k'] = w[o][i][K - 1 - k'] as [C][Cg][K]; `pad` is the FORWARD convolution's padding.  fp32 MFMA.
 * dsv_hgt_conv_wgrad: dw[row][k][ci] = sum_b sum_t g[b][row / up][t up + row % up] lrelu(x[b][ci][t + k dil - pad], slope), row < Co * up,
 *   x [B][Ci][LS(L)], g [B][Co][LS(L up)] - note the layout [rows][K][Ci].  up = 1: a convolution's weight gradient.  up = u: the weight gradient
 *   of a transposed convolution in its polyphase form (rows co * u + phase at the input rate, K and pad of that form).  Split partials on the
 *   fp32 MFMA into `workspace` (its length in floats is passed; shorter than dsv_hgt_wgrad_workspace_floats: refused), then the splits added in
 *   index order in float64, rounded once.
 * dsv_hgt_bias_grad: db[c] = sum_b sum_t g[b][c][t], float64 in a fixed order: partial sums per (channel, batch row, chunk of 1024 samples) into
 *   `workspace` (dsv_hgt_bias_workspace_floats(B, C, L) = 2 C B ceil(L / 1024) floats, 8-byte aligned, its length passed; shorter: refused), then
 *   one reduce per channel.
 * dsv_hgt_upsample_dgrad: ConvTranspose1d(Ci -> Co, kernel K, stride up, padding (K - up) / 2) behind a leaky ReLU, data gradient:
 *   dx[b][ci][q] = m(x_saved) sum_co sum_j w[ci][co][j] g[b][co][q up + j - pad] / divide; w is the plain weight [Ci][Co][K].
 * dsv_hgt_tanh_backward: out[b][t] = gy[b][t] (1 - y[b][t]^2); gy [B][L] contiguous, y / out [B][LS].
 * dsv_hgt_noise_conv_backward: dsv_noise_conv's backward from g [B][C][LS(L_out)]: dw [C][K], db [C] (float64 sums in a fixed order; db through
 *   `workspace` of dsv_hgt_bias_workspace_floats(B, C, L_out) floats like dsv_hgt_bias_grad) and dhar [B][LS(L_har)] - written when first != 0,
 *   added to otherwise (the stages accumulate in call order).
 * dsv_hgt_source_mix: sines [B][L][H] = the uv / noise mix dsv_sine_source feeds its Linear, from that call's workspace (the unmixed sines), f0
 *   and the noise draws, operation for operation.
 * dsv_hgt_source_backward: har = tanh(l_linear(sines)): dw [H] = sum dp sines, db [1] = sum dp, dp = dhar (1 - har^2); float64, fixed order. */
int32_t dsv_hgt_wgrad_split(void);
int64_t dsv_hgt_act_floats(int32_t B, int32_t C, int32_t L);
int64_t dsv_hgt_wgrad_workspace_floats(int32_t B, int32_t L, int32_t Co, int32_t Ci, int32_t K, int32_t up);
int dsv_hgt_conv_dgrad(const float* g, const float* wt_packed, const float* x_saved, const float* residual, const float* sum_in, float* dx, int32_t B,
                       int32_t Cg, int32_t C, int32_t K, int32_t pad, int32_t dil, int32_t L, float slope, float divide, void* stream);
int dsv_hgt_conv_wgrad(const float* g, const float* x, float* workspace, int64_t workspace_floats, float* dw, int32_t B, int32_t Co, int32_t Ci,
                       int32_t K, int32_t pad, int32_t dil, int32_t L, int32_t up, float slope, void* stream);
int64_t dsv_hgt_bias_workspace_floats(int32_t B, int32_t C, int32_t L);
int dsv_hgt_bias_grad(const float* g, float* workspace, int64_t workspace_floats, float* db, int32_t B, int32_t C, int32_t L, void* stream);
int dsv_hgt_upsample_dgrad(const float* g, const float* w, const float* x_saved, float* dx, int32_t B, int32_t Ci, int32_t Co, int32_t up, int32_t K,
                           int32_t L_in, float slope, float divide, void* stream);
int dsv_hgt_tanh_backward(const float* gy, const float* y, float* out, int32_t B, int32_t L, void* stream);
int dsv_hgt_noise_conv_backward(const float* g, const float* har, const float* w, float* workspace, int64_t workspace_floats, float* dw, float* db,
                                float* dhar, int32_t B, int32_t C, int32_t K, int32_t stride, int32_t pad, int32_t L_har, int32_t L_out, int32_t first,
                                void* stream);
int dsv_hgt_source_mix(const float* f0, const float* sines_ws, const float* noise, float* sines, int32_t B, int32_t T, int32_t up, int32_t H,
                       float sine_amp, float noise_std, float voiced_threshold, void* stream);
int dsv_hgt_source_backward(const float* dhar, const float* har, const float* sines, float* dw, float* db, int32_t B, int32_t L, int32_t H,
                            void* stream);

/* HiFi-GAN scale discriminator: the pooling of MultiScaleDiscriminator (modules/hifigan/hifigan.py:304-307, :316-317), forward and backward -
 * csrc/hifigan_disc.hpp.  Conventions of the section above: output rows [R][LS(L)]; every call leaves [L, LS) of its outputs at zero; no atomics, a
 * fixed order of additions (two calls are bitwise equal); nothing allocates, synchronises or reads a device value on the host; everything is
 * enqueued on `stream`; bad shapes are refused with DSD_ERR_INVALID before any launch.
 * dsv_hgd_avgpool / _backward: AvgPool1d(4, 2, padding = 1), divisor always 4 (count_include_pad), over R rows: x, rows ld_x >= L floats apart (a
 *   dense [R][L] tensor: ld_x = L; nothing is read beyond sample L of a row) -> out [R][LS(L / 2)], L >= 2, R <= 65535 (dsv_hgd_pool_samples(L) =
 *   L / 2, -1 for L < 2); the backward takes g, rows ld_g >= L / 2 floats apart, and writes dx [R][LS(L)], L the FORWARD's input length.  Input
 *   and output must not overlap. */
int32_t dsv_hgd_pool_samples(int32_t L);
int dsv_hgd_avgpool(const float* x, float* out, int64_t R, int32_t L, int64_t ld_x, void* stream);
int dsv_hgd_avgpool_backward(const float* g, float* dx, int64_t R, int32_t L, int64_t ld_g, void* stream);

/* HiFi-GAN period discriminator: DiscriminatorP (modules/hifigan/hifigan.py:181-227) forward and backward, and the feature-matching L1
 * (hifigan.py:328-334) - csrc/hifigan_mpd.hpp.  No atomics, a fixed order of additions (two calls are bitwise equal; a forward value does not depend
 * on the batch it is computed in); nothing allocates, synchronises or reads a device value on the host; everything is enqueued on `stream`; bad
 * shapes are refused with DSD_ERR_INVALID before any launch, as are overlapping input and output ranges.
 * LAYOUT: every activation is the reference's tensor, dense [B][C][H][period] float32 - no padding, no tail; a convolution runs along H only.
 *   Shapes: B >= 1, H >= 1, period in [1, 64], B * period <= 65535, B * H * period <= 2^30.  Heights: dsv_hgp_height(H, stride) = (H - 1) / stride + 1
 *   (kernel 5, padding 2).  stride is 1 or 3.
 * dsv_hgp_folded_samples(T, period): T rounded up to a multiple of the period, -1 where the reflect pad would not be shorter than T.
 * dsv_hgp_fold: F.pad(x, (0, Tp - T), 'reflect') of x, B rows ld_x >= T floats apart (nothing is read beyond sample T of a row) -> out [B][Tp],
 *   which IS [B][1][Tp / period][period].  dsv_hgp_fold_backward: g [B][Tp] -> dx [B][T]; a reflected sample's gradient adds into its source.
 * dsv_hgp_first: x [B][1][H][period], w [C][5], bias [C] or NULL -> out = leaky_relu(conv) [B][C][Ho][period].  dsv_hgp_first_backward: g0 the
 *   gradient with respect to the pre-activation -> dw [C][5], db [C] or NULL, dx [B][H][period] or NULL; workspace: dsv_hgp_edge_workspace_floats(B,
 *   Ho, period, C, 5) floats.
 * dsv_hgp_conv: a dense layer on MFMA, x [B][Ci][H][period], w_packed = dsv_pack_weight of [Co][Ci][5] (rows Co, Ci, KT 5), bias [Co] or NULL ->
 *   out = leaky_relu(conv) [B][Co][Ho][period]; Ci and Co multiples of 32.
 * dsv_hgp_conv_dgrad: g [B][Co][Ho][period] -> out [B][Ci][H][period] = (W^T g + cot) * mask(saved): cot (the cotangent arriving on the feature map
 *   below) and saved (that feature map: mask 1 where > 0, else slope) may be NULL.  Polyphase: w_packed holds, for every input phase r < stride, at
 *   float offset dsv_hgp_dgrad_packed_offset(Ci, Co, stride, r), dsv_pack_weight (rows Ci, Co, KT = number of taps) of [Ci][Co][taps] with
 *   [ci][co][t] = W[co][ci][k_t], k_t the set bits of dsv_hgp_dgrad_phase_taps(stride, r) in ascending order; offset(.., stride) is the buffer's size.
 * dsv_hgp_conv_wgrad: dw [Co][Ci][5] = sum over positions of g x, db [Co] (or NULL) = sum of g.  dsv_hgp_wgrad_splits(B, Ci, Co, Ho, period) splits
 *   of the position axis (1: no workspace, the output tiles fill the chip); workspace: dsv_hgp_wgrad_workspace_floats(..) floats (0 for one split).
 * dsv_hgp_post: a [B][C][H][period], w [C][3], bias [1] or NULL -> out [B][H][period] (kernel 3, stride 1, padding 1).  dsv_hgp_post_backward: gp
 *   (+ gp2 when not NULL: the cotangents of the flattened output and of the last feature map) -> dw [C][3], db [1] or NULL, ga [B][C][H][period] =
 *   (W^T gp + cot) * mask(a); workspace: dsv_hgp_edge_workspace_floats(B, H, period, C, 3).
 * dsv_hgp_l1_partial: dsv_hgp_l1_blocks(n) float64 partial sums of |r - g| / n into workspace (8-byte aligned); dsv_hgp_l1_final: out[0] = 2 * the
 *   sum of nblocks partials (every pair's, laid out one after the other).  dsv_hgp_l1_backward: dr = 2 sign(r - g) / n * grad_out[0], dg = -dr;
 *   sign(0) = 0. */
int32_t dsv_hgp_height(int32_t H, int32_t stride);
int64_t dsv_hgp_folded_samples(int32_t T, int32_t period);
int dsv_hgp_fold(const float* x, float* out, int32_t B, int32_t T, int64_t ld_x, int32_t period, void* stream);
int dsv_hgp_fold_backward(const float* g, float* dx, int32_t B, int32_t T, int32_t period, void* stream);
int64_t dsv_hgp_edge_workspace_floats(int32_t B, int32_t H, int32_t period, int32_t C, int32_t K);
int dsv_hgp_first(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t H, int32_t period, int32_t stride,
                  float slope, void* stream);
int dsv_hgp_first_backward(const float* g0, const float* x, const float* w, float* workspace, float* dw, float* db, float* dx, int32_t B, int32_t C,
                           int32_t H, int32_t period, int32_t stride, void* stream);
int dsv_hgp_post(const float* a, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t H, int32_t period, void* stream);
int dsv_hgp_post_backward(const float* gp, const float* gp2, const float* a, const float* w, const float* cot, float* workspace, float* dw, float* db,
                          float* ga, int32_t B, int32_t C, int32_t H, int32_t period, float slope, void* stream);
int32_t dsv_hgp_dgrad_phase_taps(int32_t stride, int32_t phase);
int64_t dsv_hgp_dgrad_packed_offset(int32_t Ci, int32_t Co, int32_t stride, int32_t phase);
int dsv_hgp_conv(const float* x, const float* w_packed, const float* bias, float* out, int32_t B, int32_t Ci, int32_t Co, int32_t H, int32_t period,
                 int32_t stride, float slope, void* stream);
int dsv_hgp_conv_dgrad(const float* g, const float* w_packed, const float* cot, const float* saved, float* out, int32_t B, int32_t Ci, int32_t Co,
                       int32_t H, int32_t period, int32_t stride, float slope, void* stream);
int32_t dsv_hgp_wgrad_splits(int32_t B, int32_t Ci, int32_t Co, int32_t H_out, int32_t period);
int64_t dsv_hgp_wgrad_workspace_floats(int32_t B, int32_t Ci, int32_t Co, int32_t H_out, int32_t period);
int dsv_hgp_conv_wgrad(const float* g, const float* x, float* workspace, float* dw, float* db, int32_t B, int32_t Ci, int32_t Co, int32_t H,
                       int32_t period, int32_t stride, void* stream);
int32_t dsv_hgp_l1_blocks(int64_t n);
int dsv_hgp_l1_partial(const float* r, const float* g, void* workspace, int64_t n, void* stream);
int dsv_hgp_l1_final(const void* workspace, int32_t nblocks, float* out, void* stream);
int dsv_hgp_l1_backward(const float* r, const float* g, const float* grad_out, float* dr, float* dg, int64_t n, void* stream);

/* HiFi-GAN scale discriminator stack: DiscriminatorS (modules/hifigan/hifigan.py:253-286) forward and backward - csrc/hifigan_msd.hpp.  Its dense
 * 1024 -> 1024 (K 5) layer and conv_post are dsv_hgp_conv / _conv_dgrad / _conv_wgrad and dsv_hgp_post / _post_backward at period 1.  No atomics, a
 * fixed order of additions (two calls are bitwise equal; a forward value and a data gradient do not depend on the batch they are computed in);
 * nothing allocates, copies, synchronises or reads a device value on the host; everything is enqueued on `stream`; bad shapes, null pointers and
 * overlapping input and output ranges are refused with DSD_ERR_INVALID before any launch.
 * LAYOUT: every activation is the reference's tensor, dense [B][C][L] float32 - no padding, no tail; nothing outside it is read or written.
 *   B in [1, 65535], L in [1, 2^30].  dsv_hgs_out_len(L, stride) = (L - 1) / stride + 1 (kernel 41, padding 20; stride 1, 2 or 4; -1 otherwise).
 * dsv_hgs_first: x, B rows ld_x >= T floats apart (nothing is read beyond sample T of a row), w [C][15], bias [C] or NULL -> out =
 *   leaky_relu(conv) [B][C][T] (padding 7).  dsv_hgs_first_backward: g0 [B][C][T] the gradient with respect to the pre-activation -> dw [C][15],
 *   db [C] or NULL, dx [B][T] or NULL; float64 sums in a fixed order; workspace: dsv_hgs_first_workspace_floats(B, T, C) floats.
 * The grouped layers: (Ci, Co, stride, groups) is one of (128, 128, 2, 4), (128, 256, 2, 16), (256, 512, 4, 16), (512, 1024, 4, 16),
 *   (1024, 1024, 1, 16); anything else is refused.  Weights are [Co][Ci / groups][41].
 * dsv_hgs_pack: w -> packed (16-byte aligned, dsv_hgs_packed_floats(Ci, Co, stride, groups, dgrad) floats): the MFMA operand stream of dsv_hgs_gconv
 *   (dgrad = 0) or of dsv_hgs_gconv_dgrad (dgrad = 1: one matrix per input phase).
 * dsv_hgs_gconv: x [B][Ci][L] -> out = leaky_relu(conv + bias) [B][Co][Lo], Lo = dsv_hgs_out_len(L, stride); bias [Co] or NULL.  fp32 MFMA, exact
 *   fp32 products; the order of an output's sum is tap, then channel.
 * dsv_hgs_gconv_dgrad: g [B][Co][Lo] -> out [B][Ci][L] = (W^T g + cot) * mask(saved), polyphase (input position stride m + r receives only the
 *   taps k = (r + 20) mod stride, + stride, ..); cot (the cotangent arriving on the feature map below) and saved (that feature map: mask 1 where
 *   > 0, else slope) may be NULL.
 * dsv_hgs_gconv_wgrad: dw [Co][Ci / groups][41] = sum over (b, q) of g[b][co][q] x[b][ci][q stride + k - 20] on the MFMA, db [Co] (or NULL) = sum of
 *   g in float64.  dsv_hgs_wgrad_splits(B, Ci, Co, Lo, stride, groups): splits of the position axis; workspace:
 *   dsv_hgs_wgrad_workspace_floats(..) floats (0 for one split). */
int32_t dsv_hgs_out_len(int32_t L, int32_t stride);
int64_t dsv_hgs_first_workspace_floats(int32_t B, int32_t T, int32_t C);
int dsv_hgs_first(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t T, int64_t ld_x, float slope,
                  void* stream);
int dsv_hgs_first_backward(const float* g0, const float* x, const float* w, float* workspace, float* dw, float* db, float* dx, int32_t B, int32_t C,
                           int32_t T, int64_t ld_x, void* stream);
int64_t dsv_hgs_packed_floats(int32_t Ci, int32_t Co, int32_t stride, int32_t groups, int32_t dgrad);
int dsv_hgs_pack(const float* w, float* packed, int32_t Ci, int32_t Co, int32_t stride, int32_t groups, int32_t dgrad, void* stream);
int dsv_hgs_gconv(const float* x, const float* w_packed, const float* bias, float* out, int32_t B, int32_t Ci, int32_t Co, int32_t L, int32_t stride,
                  int32_t groups, float slope, void* stream);
int dsv_hgs_gconv_dgrad(const float* g, const float* w_packed, const float* cot, const float* saved, float* out, int32_t B, int32_t Ci, int32_t Co,
                        int32_t L, int32_t stride, int32_t groups, float slope, void* stream);
int32_t dsv_hgs_wgrad_splits(int32_t B, int32_t Ci, int32_t Co, int32_t L_out, int32_t stride, int32_t groups);
int64_t dsv_hgs_wgrad_workspace_floats(int32_t B, int32_t Ci, int32_t Co, int32_t L_out, int32_t stride, int32_t groups);
int dsv_hgs_gconv_wgrad(const float* g, const float* x, float* workspace, float* dw, float* db, int32_t B, int32_t Ci, int32_t Co, int32_t L,
                        int32_t stride, int32_t groups, void* stream);

/* Vocoder optimisers: RAdam (modules/parallel_wavegan/optimizers/radam.py:57-89, the optimiser configs/tts/pwg.yaml configures) and AdamW
 * (torch.optim.AdamW; HiFi-GAN's adam_b1 / adam_b2) over a LIST of float32 tensors as they lie in memory, and the global L2 norm of a list of
 * gradients with clip_grad_norm_'s coefficient - csrc/voc_optim.hpp.  p, g, m, v, n are HOST arrays of `count` device pointers / element
 * counts; they are read before the call returns and need not outlive it (the tables travel in the kernel arguments: no copy to the device).
 * Any float-aligned pointer, any n[i] in [1, 2^40]; the float4 path is taken where all pointers of a tensor are 16-byte aligned.  A list longer
 * than the tables (dsv_mt_table_tensors() tensors, dsv_mt_table_chunks() chunks of dsv_mt_chunk_floats() floats per launch) is split over
 * launches.  No atomics, a fixed order of additions: two calls are bitwise equal.  Nothing allocates, synchronises or reads a device value on
 * the host; everything is enqueued on `stream`; bad arguments are refused with DSD_ERR_INVALID before any launch.
 * dsv_mt_grad_norm: out2[0] = ||g||_2 over the whole list, out2[1] = min(1, max_norm / (out2[0] + 1e-6)) in float32 (max_norm >= 0, +inf: 1);
 *   a non-finite norm propagates (NaN -> NaN, inf -> 0) as in torch.  workspace: dsv_mt_workspace_floats(n, count) floats, 8-byte aligned (one
 *   float64 partial per chunk at the chunk's index in the whole list; one workgroup adds them in ascending order): the result does not depend
 *   on how the list was split over launches.  dsv_mt_workspace_floats is host-only; -1 for a bad list.
 * dsv_mt_radam_step: with g' = g * gscale[0] when gscale (a DEVICE scalar) is not NULL: v = v b2 + ((1 - b2) g') g'; m = m b1 + (1 - b1) g';
 *   p += (-wd lr) p when wd != 0; p += ((-step_size lr) m) / (sqrt(v) + eps) when N_sma >= 5, p += (-step_size lr) m otherwise.  `step` >= 1 is the
 *   count AFTER this update.  dsv_radam_scalars (host-only): out3 = {N_sma, step_size, 1.0 when N_sma >= 5 else 0.0}, formed in double as
 *   radam.py:66-76 does.
 * dsv_mt_adamw_step: dsf_adamw_step's arithmetic (include/dsf.h) on every tensor of the list.
 * dsv_mt_set_table_limit(tensors, chunks): use fewer table entries per launch than the kernels hold (0: all of them) - process-wide, for tests
 *   that cross the launch seam at small sizes. */
int32_t dsv_mt_chunk_floats(void);
int32_t dsv_mt_table_tensors(void);
int32_t dsv_mt_table_chunks(void);
int dsv_mt_set_table_limit(int32_t tensors, int32_t chunks);
int64_t dsv_mt_workspace_floats(const int64_t* n, int64_t count);
int dsv_mt_grad_norm(const float* const* g, const int64_t* n, int64_t count, double max_norm, float* workspace, int64_t workspace_floats, float* out2,
                     void* stream);
int dsv_radam_scalars(int64_t step, double beta1, double beta2, double* out3);
int dsv_mt_radam_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int64_t count, double lr,
                      double beta1, double beta2, double eps, double weight_decay, int64_t step, const float* gscale, void* stream);
int dsv_mt_adamw_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int64_t count, double lr,
                      double beta1, double beta2, double eps, double weight_decay, int64_t step, const float* gscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSV_H */
