"""GPU: the STFT family (include/dsv.h section "STFT", csrc/voc_stft.hpp) through diffsinger_amd.stft and the vocoder classes, against the
float64 restatements of tests/stft_helpers.py (torch.stft / torch.istft on the CPU).

Bounds.  Everything that ends in a waveform: the project's 2e-5 (tests/test_vocoder_host.py:248).  Spectra, magnitudes and mels: 2 x the
error of `yardstick32` - the same contraction as a float32 torch.matmul on the CPU - against the same float64 reference on the test's own
input, computed inside the test: kernel and yardstick are fp32 sums of the same products in a different order.  Every test prints its
measured maximum next to its bound (recorded in profiles/stft_pytest_gpu.txt)."""
import numpy as np
import pytest
import torch

from diffsinger_amd import _lib
from diffsinger_amd import stft as ST
from diffsinger_amd import vocoder as V
from diffsinger_amd.graphs import GraphedForward
from diffsinger_amd.hparams import hparams
from tests import stft_helpers as SH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WAV_TOL = 2e-5
SHAPES = [(512, 128, 512), (1024, 256, 1024), (1024, 256, 800), (2048, 512, 2048), (256, 64, 256)]
SHIPPED = {512: (24000, 80, 50, 11025), 1024: (22050, 80, 80, 7600)}      # n_fft -> (sample rate, mel bins, fmin, fmax) of the shipped configs


def _cerr(got, want):
    """max-abs over re and im of complex tensors"""
    d = torch.view_as_real(got.to(torch.complex128).cpu()) - torch.view_as_real(want.to(torch.complex128))
    return float(d.abs().max())


@pytest.fixture
def clean_hparams():
    saved = dict(hparams)
    hparams.clear()
    yield hparams
    hparams.clear()
    hparams.update(saved)


@pytest.mark.parametrize('n_fft,hop,win', SHAPES)
def test_forward_against_float64(n_fft, hop, win):
    worst = 0.0
    for L in (n_fft - 1, n_fft, 9000, 24000):
        wav = SH.make_signal(L, seed=L)
        for mode in ('constant', 'reflect'):
            for center in (True, False):
                if L == n_fft - 1 and not (center and mode == 'constant'):
                    continue                                                 # shorter than a frame: only the centred, zero-padded form has frames
                want = SH.ref_stft64(wav, n_fft, hop, win, center, mode)
                yard = _cerr(SH.yardstick32(wav, n_fft, hop, win, center, mode), want)
                got = ST.stft_op(wav.to(DEV), n_fft=n_fft, hop=hop, win_length=win, center=center, pad_mode=mode)
                assert got.shape == want.shape and got.dtype == torch.complex64
                err = _cerr(got, want)
                worst = max(worst, err / yard)
                print(f'stft {n_fft}/{hop}/{win} L={L} {mode} center={int(center)}: {want.shape[2]} frames, max-abs err {err:.3e}, CPU fp32 yardstick {yard:.3e}')
                assert err <= 2 * yard, (L, mode, center, err, yard)
    print(f'stft {n_fft}/{hop}/{win}: worst err / yardstick {worst:.2f}')


def test_forward_large_batch_one_row_checked():
    n_fft, hop, win = 1024, 256, 1024
    wav = SH.make_signal(262144, seed=11, batch=8)
    got = ST.stft_op(wav.to(DEV), n_fft=n_fft, hop=hop, win_length=win)
    assert got.shape == (8, 513, 1025) and bool(torch.isfinite(torch.view_as_real(got)).all())
    r = 5
    want = SH.ref_stft64(wav[r], n_fft, hop, win)
    yard = _cerr(SH.yardstick32(wav[r], n_fft, hop, win), want)
    err = _cerr(got[r:r + 1], want)
    print(f'stft 8 x 262144, row {r}: max-abs err {err:.3e}, CPU fp32 yardstick {yard:.3e}')
    assert err <= 2 * yard
    solo = ST.stft_op(wav[r:r + 1].to(DEV), n_fft=n_fft, hop=hop, win_length=win)
    assert torch.equal(torch.view_as_real(solo), torch.view_as_real(got[r:r + 1]))          # rows are independent of the batch around them


@pytest.mark.parametrize('mode', ['constant', 'reflect'])
def test_forward_ragged_batch(mode):
    n_fft, hop, win, L = 512, 128, 512, 9000
    lens = [9000, 5000, 700, 0]
    wav = SH.make_signal(L, seed=3, batch=4)
    got, fc = ST.stft_op(wav.to(DEV), n_fft=n_fft, hop=hop, win_length=win, pad_mode=mode, lengths=torch.tensor(lens), return_frames=True)
    T = 1 + L // hop
    assert got.shape == (4, 257, T) and fc.dtype == torch.int32
    assert fc.cpu().tolist() == [1 + n // hop if n else 0 for n in lens]
    for b, n in enumerate(lens):
        t = int(fc[b])
        assert not bool(torch.view_as_real(got[b, :, t:]).any())                               # frames beyond the row's count: exactly 0
        if n:
            want = SH.ref_stft64(wav[b, :n], n_fft, hop, win, True, mode)
            yard = _cerr(SH.yardstick32(wav[b, :n], n_fft, hop, win, True, mode), want)
            err = _cerr(got[b:b + 1, :, :t], want)
            print(f'ragged {mode} row {b} ({n} samples, {t} frames): max-abs err {err:.3e}, yardstick {yard:.3e}')
            assert err <= 2 * yard


def test_denoise_post_filter():
    from diffsinger_amd.vocoder import denoise
    for n_fft, hop, win, n in ((512, 128, 512, 24000), (1024, 256, 1024, 22050), (1024, 256, 800, 9000)):
        wav = SH.make_signal(n, seed=4)
        for v in (0.0, 0.1, 0.5):
            got = ST.denoise_op(wav.to(DEV)[None], v, fft_size=n_fft, hop_size=hop, win_size=win)[0].cpu().numpy()
            want = SH.ref_denoise64(wav, v, n_fft, hop, win).numpy()
            host = denoise(wav.numpy(), v=v, fft_size=n_fft, hop_size=hop, win_size=win)
            assert len(got) == len(host) == hop * (n // hop)                                    # the same length exactly
            m = min(len(got), len(want))
            edge = n_fft
            e_ref = float(np.abs(got[edge:m - edge] - want[edge:m - edge]).max())
            e_host = float(np.abs(got - host).max())                                            # the whole length, edges included
            print(f'denoise {n_fft}/{hop}/{win} v={v}: interior err vs float64 {e_ref:.3e}, whole-length err vs the host function {e_host:.3e} (bound {WAV_TOL})')
            assert e_ref < WAV_TOL and e_host < WAV_TOL
            if v == 0.0:
                e_id = float(np.abs(got[edge:m - edge] - wav.numpy()[edge:m - edge]).max())
                print(f'   v=0 identity err {e_id:.3e}')
                assert e_id < WAV_TOL
    # a ragged batch: every row is the filter of its own valid samples, 0 behind them
    n_fft, hop, win = 512, 128, 512
    wav = SH.make_signal(6000, seed=8, batch=3).to(DEV)
    lens = [6000, 4100, 1000]
    got = ST.denoise_op(wav, 0.1, fft_size=n_fft, hop_size=hop, win_size=win, lengths=torch.tensor(lens))
    for b, n in enumerate(lens):
        solo = ST.denoise_op(wav[b:b + 1, :n], 0.1, fft_size=n_fft, hop_size=hop, win_size=win)
        assert torch.equal(got[b, :solo.shape[1]], solo[0]) and not bool(got[b, solo.shape[1]:].any())


def test_spec2wav_post_filter_on_the_device(clean_hparams):
    from oracle import hifigan_oracle as HO
    from oracle.make_golden_hifigan import CONFIG
    h = dict(CONFIG, use_pitch_embed=False)
    m = V.HifiGanGenerator(h)
    m.load_state_dict(HO.synth_generator_params(h, 1234), strict=True)
    voc = V.HifiGAN(m.to(DEV), DEV, use_nsf=False)
    mel = torch.randn(40, 80, generator=torch.Generator().manual_seed(2)).numpy()
    try:
        for c in (0.1, 0.0):
            hparams.clear()
            hparams.update(vocoder_denoise_c=c, fft_size=1024, hop_size=256, win_size=1024)
            V.set_denoise_native(True)
            native = voc.spec2wav(mel)
            V.set_denoise_native(False)
            host = voc.spec2wav(mel)
            assert native.dtype == host.dtype == np.float32 and native.shape == host.shape == (40 * 256,)
            if c > 0:
                err = float(np.abs(native - host).max())
                print(f'spec2wav vocoder_denoise_c={c}: native vs host post-filter max-abs {err:.3e} (bound {WAV_TOL}); |wav| max {np.abs(host).max():.3f}')
                assert err < WAV_TOL
            else:
                assert np.array_equal(native, host)
    finally:
        V.set_denoise_native(True)


def _mel_basis(n_fft):
    sr, M, fmin, fmax = SHIPPED[n_fft]
    return ST.mel_filterbank(sr, n_fft, M, fmin, fmax)


@pytest.mark.parametrize('flavour', ['pwg', 'hifigan'])
@pytest.mark.parametrize('n_fft,hop,win', [(512, 128, 512), (1024, 256, 1024)])
def test_logmel_against_float64(flavour, n_fft, hop, win):
    """Log-domain comparison under the condition that the float64 mel is >= 1e-3 in every bin of every frame (asserted on the reference: an fp32
    error of 1e-6 in a bin at the 1e-10 floor is four decades in the log and says nothing about the kernel).  The operator does not return
    the linear mel; the linear MAGNITUDE (return_linear) is checked against its own yardstick instead."""
    basis = _mel_basis(n_fft)
    assert (basis.max(axis=1) > 0).all()                                      # no all-zero basis row at the shipped shapes: no bin is exempt
    for B, L in ((1, 9000), (3, 24000)):
        # noise floor 0.3: at 24 kHz / 512 the lowest mel filters hold ONE bin each, and with the 0.1 of the waveform tests a single Rayleigh-distributed
        # magnitude falls below the 1e-3 condition in some frame (float64 reference: 2.8e-4 .. 9.4e-4)
        wav = SH.make_signal(L, seed=L + n_fft, batch=B, noise=0.3) * (1.3 if flavour == 'hifigan' else 1.0)      # the hifigan form clamps: let samples clip
        want, want_mel, want_mag = SH.ref_logmel64(wav, basis, flavour, n_fft, hop, win)
        assert float(want_mel.min()) >= 1e-3, float(want_mel.min())
        y_log, _, y_mag = SH.yardstick32(wav, n_fft, hop, win, basis=basis, flavour=flavour)
        yard = float((y_log.double() - want).abs().max())
        yard_mag = float((y_mag.double() - want_mag).abs().max())
        got, lin = ST.logmel_op(wav.to(DEV), torch.from_numpy(basis).to(DEV), n_fft=n_fft, hop=hop, win_length=win, flavour=flavour, return_linear=True)
        assert got.shape == want.shape and lin.shape == want_mag.shape
        err = float((got.cpu().double() - want).abs().max())
        err_mag = float((lin.cpu().double() - want_mag).abs().max())
        print(f'logmel {flavour} {n_fft}/{hop} B={B} L={L}: log-domain err {err:.3e} (yardstick {yard:.3e}), magnitude err {err_mag:.3e} (yardstick {yard_mag:.3e}), min mel {float(want_mel.min()):.3e}')
        assert err <= 2 * yard and err_mag <= 2 * yard_mag
        only = ST.logmel_op(wav.to(DEV), torch.from_numpy(basis).to(DEV), n_fft=n_fft, hop=hop, win_length=win, flavour=flavour)
        assert torch.equal(only, got)                                         # the optional output does not change the mel


def test_logmel_floor_and_ragged_rows():
    n_fft, hop = 1024, 256
    basis = torch.from_numpy(_mel_basis(n_fft)).to(DEV)
    zero = torch.zeros(2, 5000, device=DEV)
    out = ST.logmel_op(zero, basis, n_fft=n_fft, hop=hop, flavour='pwg', eps=1e-10)
    assert out.shape == (2, 20, 80)
    assert float(np.float32(np.log10(1e-10))) == -10.0
    assert bool((out == -10.0).all())                                          # an all-zero utterance: exactly float32(log10(eps)) everywhere
    out = ST.logmel_op(zero, basis, n_fft=n_fft, hop=hop, flavour='hifigan')
    # sqrt(1e-9) * sum(basis row) < 1e-5: the floor, which the operator receives as a float32 - float32(ln(float32(1e-5))) exactly
    assert bool((out == float(np.float32(np.log(np.float64(np.float32(1e-5)))))).all())
    wav = SH.make_signal(9000, seed=6, batch=3).to(DEV)
    lens = [9000, 4000, 0]
    got, fc = ST.logmel_op(wav, basis, n_fft=n_fft, hop=hop, flavour='pwg', lengths=torch.tensor(lens), return_frames=True)
    assert fc.cpu().tolist() == [36, 16, 0]
    for b, n in enumerate(lens):
        t = int(fc[b])
        assert not bool(got[b, t:].any())                                      # frames beyond the row's count: exactly 0, the padding value of mels
        if n:
            solo = ST.logmel_op(wav[b:b + 1, :n], basis, n_fft=n_fft, hop=hop, flavour='pwg')
            assert torch.equal(solo[0], got[b, :t])


@pytest.mark.parametrize('n_fft', [512, 1024])
def test_wav2spec_is_process_utterance(n_fft, clean_hparams, tmp_path):
    sr, M, fmin, fmax = SHIPPED[n_fft]
    hop = n_fft // 4
    hparams.update(fft_size=n_fft, hop_size=hop, win_size=n_fft, audio_num_mel_bins=M, fmin=fmin, fmax=fmax, audio_sample_rate=sr, min_level_db=-100,
                   loud_norm=False)
    basis = ST.mel_filterbank(sr, n_fft, M, fmin, fmax)
    from diffsinger_amd.pwg import PWG
    reg = {}
    V.register_vocoders(reg)
    for n in (hop * 40 - 1, hop * 40, hop * 40 + 1, 9000):
        wav = SH.make_signal(n, seed=n, noise=0.3).numpy()                       # the noise floor of test_logmel_against_float64
        w_ref, mel_ref, spc_ref = SH.ref_process_utterance64(wav, basis, n_fft, hop, n_fft, return_linear=True)
        ref_log, ref_mel, ref_mag = SH.ref_logmel64(wav[None], basis, 'pwg', n_fft, hop, n_fft)
        assert float(ref_mel.min()) >= 1e-3
        y_log, _, y_mag = SH.yardstick32(wav[None], n_fft, hop, n_fft, basis=basis, flavour='pwg')
        yard = float((y_log.double() - ref_log).abs().max())
        eps_mag = 2 * float((y_mag.double() - ref_mag).abs().max())
        for cls in (reg['pwg'], reg['hifigan']):
            w, mel = cls.wav2spec(wav)
            assert w.dtype == mel.dtype == np.float32 and mel.shape == mel_ref.shape == (n // hop + 1, M)
            assert np.array_equal(w, w_ref)                                    # the returned waveform: exact
            err = float(np.abs(mel - mel_ref).max())
            assert err <= 2 * yard, (err, yard)
        w, mel2, spc = PWG.wav2spec(wav, return_linear=True)
        assert np.array_equal(w, w_ref) and np.array_equal(mel2, mel) and spc.dtype == np.float32 and spc.shape == spc_ref.shape
        # spc = (20 log10(max(1e-5, mag)) + 100) / 100: d spc / d mag = 20 / (100 ln 10 mag); a magnitude error of eps_mag (2 x the yardstick's) moves
        # an element by at most that slope at (mag - eps_mag), plus the float32 rounding of the log and of the result (spc is O(1): 1e-6)
        slope = 20.0 / (100.0 * np.log(10.0)) / np.maximum(ref_mag[0].numpy() - eps_mag, 1e-5)
        excess = float((np.abs(spc - spc_ref) - (slope * eps_mag + 1e-6)).max())
        print(f'wav2spec {n_fft}/{hop} n={n}: mel log-domain err {err:.3e} (yardstick {yard:.3e}); linear dB-normalised err {float(np.abs(spc - spc_ref).max()):.3e}, '
              f'worst element {excess:.3e} against its own bound (<= 0)')
        assert excess <= 0
        dev = reg['pwg'].wav2spec_batch(torch.from_numpy(wav).to(DEV)[None])
        assert dev.is_cuda and np.array_equal(dev[0].cpu().numpy(), mel)       # the device-resident form: the same launch
    # a WAV file at the configured rate goes through the same path
    import wave
    pcm = (SH.make_signal(5000, seed=1).numpy() * 32767).astype('<i2')
    with wave.open(str(tmp_path / 'a.wav'), 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())
    w_file, mel_file = PWG.wav2spec(str(tmp_path / 'a.wav'))
    w_arr, mel_arr = PWG.wav2spec(pcm.astype(np.float32) / 32768.0)
    assert np.array_equal(w_file, w_arr) and np.array_equal(mel_file, mel_arr)


@pytest.mark.parametrize('n_fft,hop,win', SHAPES)
def test_round_trip(n_fft, hop, win):
    L = 24000
    wav = SH.make_signal(L, seed=21)
    S64 = SH.ref_stft64(wav, n_fft, hop, win)
    back64 = SH.ref_istft64(S64, n_fft, hop, win)
    m = back64.shape[-1]
    edge = n_fft
    e64 = float((back64[0, edge:m - edge] - wav[edge:m - edge].double()).abs().max())
    assert e64 < 1e-9, e64                                                     # the float64 reference's own round trip holds on this input
    S = ST.stft_op(wav.to(DEV), n_fft=n_fft, hop=hop, win_length=win)
    back = ST.istft_op(S, n_fft=n_fft, hop=hop, win_length=win)[0].cpu()
    assert back.shape[0] == m == hop * (L // hop)
    err = float((back[edge:m - edge] - wav[edge:m - edge]).abs().max())
    print(f'round trip {n_fft}/{hop}/{win}: interior max-abs {err:.3e} (bound {WAV_TOL}; float64 reference {e64:.1e})')
    assert err < WAV_TOL


def test_determinism_and_graph_capture(monkeypatch):
    n_fft, hop = 1024, 256
    basis = torch.from_numpy(_mel_basis(n_fft)).to(DEV)
    a = SH.make_signal(16384, seed=31, batch=2).to(DEV)
    b = SH.make_signal(16384, seed=32, batch=2).to(DEV)
    f_mel = lambda w: ST.logmel_op(w, basis, n_fft=n_fft, hop=hop, flavour='pwg')                          # noqa: E731
    f_den = lambda w: ST.denoise_op(w, 0.1, fft_size=n_fft, hop_size=hop, win_size=n_fft)                  # noqa: E731
    f_spec = lambda w: torch.view_as_real(ST.stft_op(w, n_fft=n_fft, hop=hop, pad_mode='reflect'))         # noqa: E731
    for f in (f_mel, f_den, f_spec):
        assert torch.equal(f(a), f(a))                                         # two calls: bitwise equal
    for name, f in (('logmel_op', f_mel), ('denoise_op', f_den)):
        eager_b = f(b).clone()
        g = GraphedForward(f)
        first = g(a).clone()
        assert torch.equal(first, f(a))
        replay = g(b).clone()                                                  # captured once on `a`, replayed on another waveform of the same shape
        assert g.captures == 1 and torch.equal(replay, eager_b), name
        print(f'{name}: graph replay carries the bits of the eager call')
    # the one-time basis build is refused while a capture is under way instead of being recorded into it (no capture is opened for this:
    # the question the library asks torch is answered for it)
    ST._BASES.pop((0, 256, 200), None)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='graph'):
        ST.bases(DEV, 256, 200)
    assert (0, 256, 200) not in ST._BASES


def test_refusals():
    """Argument errors only: each is raised on the host, nothing is launched."""
    x = torch.zeros(1, 4096, device=DEV)
    basis = torch.zeros(80, 513, device=DEV)
    cases = [
        (lambda: ST.stft_op(x, n_fft=1000, hop=250), 'n_fft=1000'),
        (lambda: ST.stft_op(x, n_fft=4096, hop=1024), 'n_fft=4096'),
        (lambda: ST.stft_op(x, n_fft=1024, hop=256, win_length=1025), 'win_length=1025'),
        (lambda: ST.stft_op(x, n_fft=1024, hop=0), 'hop=0'),
        (lambda: ST.stft_op(x, n_fft=1024, hop=1025), 'hop=1025'),
        (lambda: ST.stft_op(x[:, :1023], n_fft=1024, hop=256, center=False), 'shorter than one frame'),
        (lambda: ST.stft_op(x[:, :400], n_fft=1024, hop=256, pad_mode='reflect'), 'reflect padding'),
        (lambda: ST.logmel_op(x, torch.zeros(129, 513, device=DEV), n_fft=1024, hop=256), 'M=129'),
        (lambda: ST.logmel_op(x, basis[:, :512], n_fft=1024, hop=256), 'mel_basis'),
        (lambda: ST.logmel_op(x[:, :100], basis, n_fft=1024, hop=256, flavour='hifigan'), 'reflect padding'),
        (lambda: ST.denoise_op(x, -0.1, fft_size=1024, hop_size=256, win_size=1024), 'subtract'),
        (lambda: ST.istft_op(torch.zeros(1, 512, 8, dtype=torch.complex64, device=DEV), n_fft=1024, hop=256), 'spectrum must be'),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fn()
    # the C ABI refuses the same cases itself (DSD_ERR_INVALID = -1, message in dsd_last_error), before any launch
    lib = _lib.load()
    spec = torch.empty(1, 513, 17, 2, device=DEV)
    fwd, inv = ST.bases(DEV, 1024, 1024)
    s = torch.cuda.current_stream().cuda_stream
    for args, msg in (((1, 4096, 1000, 250, 500, 500, 0, 0, 0.0), b'n_fft=1000'), ((1, 4096, 1024, 0, 512, 512, 0, 0, 0.0), b'hop=0'),
                      ((1, 1023, 1024, 256, 0, 0, 0, 0, 0.0), b'shorter than one frame'), ((1, 4096, 1024, 256, 512, 512, 2, 0, 0.0), b'pad_mode'),
                      ((70000, 4096, 1024, 256, 512, 512, 0, 0, 0.0), b'B=70000')):
        assert lib.dsv_stft(x.data_ptr(), None, fwd.data_ptr(), spec.data_ptr(), None, *args, s) == -1
        assert msg in lib.dsd_last_error(), (msg, lib.dsd_last_error())
    assert lib.dsv_logmel(x.data_ptr(), None, fwd.data_ptr(), basis.data_ptr(), spec.data_ptr(), None, None, 1, 4096, 1024, 256, 512, 512, 0, 0, 129, 0.0, 1e-5, 0, s) == -1
    assert b'M=129' in lib.dsd_last_error()
    assert lib.dsv_stft_make_basis(1024, 1025, fwd.data_ptr(), None, s) == -1 and b'win_length=1025' in lib.dsd_last_error()
    assert lib.dsv_stft_basis_floats(768, 0) == -1 and lib.dsv_stft_frames(1023, 1024, 256, 0, 0) == -1
    assert lib.dsv_stft_frames(22050, 1024, 256, 512, 512) == 87 and lib.dsv_istft_samples(87, 1024, 256, 1) == 86 * 256
    torch.cuda.synchronize()
