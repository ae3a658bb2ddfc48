"""CPU: the host side of the STFT family (diffsinger_amd/stft.py) - the mel filterbank against its published definition, the float64 test
helpers' frame arithmetic, wav2spec's argument handling, and the presence of wav2spec on the vocoder classes and behind register_vocoders.
No GPU: nothing here launches a kernel."""
import os
import wave

import numpy as np
import pytest
import torch

from diffsinger_amd import stft as ST
from diffsinger_amd.hparams import hparams
from tests import stft_helpers as SH

SHIPPED = [(22050, 1024, 80, 80, 7600), (24000, 512, 80, 50, 11025)]          # configs/tts/base.yaml:38-47, configs/singing/base.yaml:17-26
OTHERS = [(22050, 1024, 80, 0, 11025.0), (16000, 256, 40, 0, 8000.0), (44100, 2048, 128, 40, 16000)]


@pytest.fixture
def clean_hparams():
    saved = dict(hparams)
    hparams.clear()
    yield hparams
    hparams.clear()
    hparams.update(saved)


def _edges(n_mels, fmin, fmax):
    return ST.mel_to_hz(np.linspace(ST.hz_to_mel(fmin), ST.hz_to_mel(fmax), n_mels + 2))


def test_slaney_scale_fixed_points():
    assert float(ST.hz_to_mel(0.0)) == 0.0 and abs(float(ST.hz_to_mel(1000.0)) - 15.0) < 1e-12      # 1000 / (200 / 3) in float64, as librosa forms it
    assert abs(float(ST.hz_to_mel(200.0 / 3)) - 1.0) < 1e-12
    assert abs(float(ST.hz_to_mel(6400.0)) - 42.0) < 1e-9                     # 27 log steps of log(6.4) / 27 above 1 kHz
    f = np.array([0.0, 55.0, 999.9, 1000.0, 1000.1, 7600.0, 11025.0])
    assert float(np.abs(ST.mel_to_hz(ST.hz_to_mel(f)) - f).max()) < 1e-9


@pytest.mark.parametrize('sr,n_fft,n_mels,fmin,fmax', SHIPPED + OTHERS)
def test_mel_filterbank_is_the_published_definition(sr, n_fft, n_mels, fmin, fmax):
    B = ST.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    n_bins = n_fft // 2 + 1
    assert B.shape == (n_mels, n_bins) and B.dtype == np.float32
    assert float(B.min()) >= 0.0
    freqs = np.arange(n_bins) * (sr / n_fft)
    df = sr / n_fft
    edges = _edges(n_mels, fmin, fmax)
    outside = (freqs < fmin) | (freqs > fmax)
    assert float(B[:, outside].max(initial=0.0)) == 0.0
    centres = []
    for m in range(n_mels):
        row = B[m].astype(np.float64)
        # zero outside its own three edges, one triangle inside: a single maximum, monotone on both sides
        assert not row[(freqs <= edges[m]) | (freqs >= edges[m + 2])].any()
        if row.any():
            k = int(row.argmax())
            assert np.all(np.diff(row[:k + 1]) >= 0) and np.all(np.diff(row[k:]) <= 0), m
            centres.append(float((row * freqs).sum() / row.sum()))
        # Slaney normalisation: the continuous triangle has unit area; the bin grid samples it with spacing df, and the trapezoid rule on a
        # piecewise-linear function errs only in the three intervals that hold a kink, by at most df^2 / 8 x the slope change there:
        # df^2 / 8 * 2 h (1 / (c - lo) + 1 / (hi - c)), h = 2 / (hi - lo) the peak (+ float32 rounding of the n_bins entries)
        lo, c, hi = edges[m], edges[m + 1], edges[m + 2]
        h = 2.0 / (hi - lo)
        bound = df * df / 4.0 * h * (1.0 / (c - lo) + 1.0 / (hi - c)) + 1e-6
        assert abs(row.sum() * df - 1.0) <= bound, (m, row.sum() * df, bound)
    assert centres == sorted(centres) and len(set(centres)) == len(centres)                   # filters ordered
    if (sr, n_fft, n_mels, fmin, fmax) in SHIPPED:
        # at 24 kHz / 512 the mel step at the bottom is ~40 Hz against a bin spacing of 46.9 Hz: the lowest filters hold one or two bins each,
        # none is empty (librosa's "empty filters" warning case does not arise at either shipped shape)
        assert int((B.max(axis=1) == 0).sum()) == 0
        print(f'{sr}/{n_fft}/{n_mels}/{fmin}-{fmax}: bins per filter min {int((B > 0).sum(axis=1).min())}, max {int((B > 0).sum(axis=1).max())}')


def test_minus_one_means_the_whole_band(clean_hparams):
    hparams.update(fft_size=512, hop_size=128, win_size=512, audio_num_mel_bins=80, fmin=-1, fmax=-1, audio_sample_rate=24000, min_level_db=-120)
    q = ST._wav2spec_params(hparams)
    assert q['fmin'] == 0 and q['fmax'] == 12000 and q['eps'] == 1e-10


@pytest.mark.parametrize('hop', [128, 256])
def test_reference_helper_frame_arithmetic(hop):
    n_fft = 4 * hop
    basis = ST.mel_filterbank(22050, n_fft, 80, 80, 7600)
    for n in (hop * 9 - 1, hop * 9, hop * 9 + 1, hop * 12 - 1, hop * 12, hop * 12 + 1):
        wav = SH.make_signal(n).numpy()
        w, mel, spc = SH.ref_process_utterance64(wav, basis, n_fft, hop, n_fft, return_linear=True)
        T = n // hop + 1
        assert mel.shape == (T, 80) and spc.shape == (T, n_fft // 2 + 1) and w.shape == (T * hop,)
        assert np.array_equal(w[:n], wav) and not w[n:].any()


def test_yardstick_is_close_to_the_float64_reference():
    """The yardstick shares only the definition with the reference: a wrong basis in it would make every GPU bound meaningless."""
    for n_fft, hop, win in ((512, 128, 512), (1024, 256, 800)):
        wav = SH.make_signal(9000)
        for mode, center in (('constant', True), ('reflect', True), ('reflect', False)):
            want = SH.ref_stft64(wav, n_fft, hop, win, center, mode)
            got = SH.yardstick32(wav, n_fft, hop, win, center, mode)
            assert got.shape == want.shape
            assert float((got.to(torch.complex128) - want).abs().max()) < 1e-3 * float(want.abs().max())


def _write_wav(path, sr, n=4000):
    pcm = (np.sin(np.arange(n) * 0.05) * 8000).astype('<i2')
    with wave.open(str(path), 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())
    return pcm


def test_wav2spec_argument_handling(clean_hparams, tmp_path):
    full = dict(fft_size=1024, hop_size=256, win_size=1024, audio_num_mel_bins=80, fmin=80, fmax=7600, audio_sample_rate=22050, min_level_db=-100)
    wav = np.zeros(5000, np.float32)
    for k in full:                                                                           # a missing hparam: KeyError naming it
        hparams.clear()
        hparams.update({kk: v for kk, v in full.items() if kk != k})
        with pytest.raises(KeyError, match=k):
            ST.wav2spec(wav)
    hparams.clear()
    hparams.update(full, loud_norm=True)
    with pytest.raises(NotImplementedError, match='pyloudnorm'):
        ST.wav2spec(wav)
    hparams.update(loud_norm=False, trim_long_sil=True)
    with pytest.raises(NotImplementedError, match='webrtcvad'):
        ST.wav2spec(wav)
    hparams.update(trim_long_sil=False)
    p = tmp_path / 'a.wav'
    pcm = _write_wav(p, 16000)
    with pytest.raises(ValueError, match=r'16000.*22050'):
        ST.wav2spec(str(p))
    _write_wav(p, 22050)
    got = ST.read_wav(str(p), 22050)
    assert got.dtype == np.float32 and np.array_equal(got, pcm.astype(np.float32) / 32768.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            ST.wav2spec(wav)


def test_operator_argument_errors_need_no_device():
    x = torch.zeros(1, 4096)
    for kw, msg in ((dict(n_fft=1000, hop=250), 'n_fft=1000'), (dict(n_fft=1024, hop=0), 'hop=0'), (dict(n_fft=1024, hop=2048), 'hop=2048'),
                    (dict(n_fft=1024, hop=256, win_length=1025), 'win_length=1025')):
        with pytest.raises(ValueError, match=msg):
            ST.stft_op(x, **kw)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ST.stft_op(x, n_fft=1024, hop=256)


def test_vocoder_classes_carry_wav2spec_and_the_registry_reaches_it(clean_hparams):
    """vocoders/base_vocoder.py:22-39: the interface is spec2wav AND wav2spec; the reference's binarizers call
    VOCODERS[hparams['vocoder']].wav2spec(wav_fn) on the CLASS (data_gen/tts/base_binarizer.py:162-164)."""
    from diffsinger_amd import vocoder as V
    from diffsinger_amd.pwg import PWG
    reg = {}
    V.register_vocoders(reg)
    for name, cls in (('pwg', PWG), ('PWG', PWG), ('hifigan', V.HifiGAN), ('HifiGAN', V.HifiGAN)):
        assert reg[name] is cls
        assert callable(reg[name].wav2spec) and callable(reg[name].wav2spec_batch)
        assert not hasattr(reg[name], 'wav2mfcc')
        with pytest.raises(KeyError, match='fft_size'):                                     # reached diffsinger_amd.stft.wav2spec: no hparams are set
            reg[name].wav2spec(np.zeros(3000, np.float32))
    assert V.get_vocoder_cls({'vocoder': 'pwg'}).wav2spec is PWG.wav2spec
    V.set_denoise_native(False)
    assert V._DENOISE_NATIVE['on'] is False
    V.set_denoise_native(True)
    assert V._DENOISE_NATIVE['on'] is True
