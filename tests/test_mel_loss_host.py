"""CPU: the host side of the mel loss (include/dsv.h, section "Mel loss") - the header, the binding and the library's exports, every refusal
of the C ABI (nothing is launched: fake addresses, null stream), the float64 formula of the head's vector-Jacobian product
(tests/mel_loss_helpers.py) against autograd, and the Python refusals that must hold on a host without a device.  The kernels themselves are
checked on the GPU (tests/test_gpu_mel_loss.py)."""
import numpy as np
import pytest
import torch

from diffsinger_amd import _lib
from tests import mel_loss_helpers as MH
from tests import stft_helpers as SH

NEW = ['dsv_mel_spectrum', 'dsv_mel_head', 'dsv_mel_head_backward', 'dsv_mel_clamp_backward']
A, Bp, Cp, Dp, Ep = (0x10000000 * (i + 1) for i in range(5))               # fake, aligned, far apart: never dereferenced


def test_header_binding_and_exports():
    from tests.test_abi import _header_symbols
    hdr = _header_symbols('dsv.h', 'dsv_')
    lib = _lib.load()
    for name in NEW:
        assert name in hdr and name in _lib.SYMBOLS_VOC and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.dsd_abi_version() == 8


def _refused(lib, name, *args):
    rc = getattr(lib, name)(*args, None)
    msg = lib.dsd_last_error().decode()
    assert rc == -1 and name + ':' in msg, (name, args, rc, msg)
    return msg


def test_head_refusals():
    lib = _lib.load()
    ok = dict(B=2, T=33, n_fft=512, M=80, mag_eps=1e-9, floor=1e-5, log10=0)

    def fwd(spec=A, basis=Bp, out=Cp, mel=Dp, **kw):
        q = dict(ok, **kw)
        return _refused(lib, 'dsv_mel_head', spec, basis, out, mel, q['B'], q['T'], q['n_fft'], q['M'], q['mag_eps'], q['floor'], q['log10'])

    def bwd(spec=A, basis=Bp, g=Cp, mel=Dp, G=Ep, **kw):
        q = dict(ok, **kw)
        return _refused(lib, 'dsv_mel_head_backward', spec, basis, g, mel, G, q['B'], q['T'], q['n_fft'], q['M'], q['mag_eps'], q['floor'], q['log10'])

    for f, ptrs in ((fwd, ('spec', 'basis', 'out', 'mel')), (bwd, ('spec', 'basis', 'g', 'mel', 'G'))):
        for p in ptrs:
            assert 'null' in f(**{p: None})
        for n_fft in (0, 128, 500, 4096):
            assert 'n_fft' in f(n_fft=n_fft)
        for M in (0, 129, -1):
            assert 'M=' in f(M=M)
        assert 'T=' in f(T=0)
        for B in (0, 65536):
            assert 'B=' in f(B=B)
        for kw in (dict(mag_eps=-1e-9), dict(floor=0.0), dict(floor=-1.0), dict(mag_eps=float('inf')), dict(floor=float('inf')),
                   dict(mag_eps=float('nan')), dict(floor=float('nan'))):
            assert 'finite' in f(**kw), kw
    ns, nw, no = 2 * 257 * 33 * 2 * 4, 80 * 257 * 4, 2 * 33 * 80 * 4      # bytes of the spectrum, the basis, an output
    assert 'overlap' in fwd(out=A + ns - 4) and 'overlap' in fwd(out=Bp + nw - 4) and 'overlap' in fwd(mel=A) and 'overlap' in fwd(mel=Cp + no - 4)
    assert 'overlap' in fwd(out=A - no + 4)
    for inp in (A, Bp, Cp, Dp):
        assert 'overlap' in bwd(G=inp)
    assert 'overlap' in bwd(G=Cp - ns + 8) and 'overlap' in bwd(G=Dp + no - 8)
    assert 'aligned' in fwd(spec=A + 4) and 'aligned' in bwd(G=Ep + 4)


def test_spectrum_and_clamp_backward_refusals():
    lib = _lib.load()
    ok = dict(B=2, L=4096, n_fft=512, hop=128, pl=192, pr=192, mode=1, clamp=1)

    def spec(wav=A, basis=Bp, out=Cp, **kw):
        q = dict(ok, **kw)
        return _refused(lib, 'dsv_mel_spectrum', wav, basis, out, q['B'], q['L'], q['n_fft'], q['hop'], q['pl'], q['pr'], q['mode'], q['clamp'])
    for p in ('wav', 'basis', 'out'):
        assert 'null' in spec(**{p: None})
    assert 'n_fft' in spec(n_fft=384) and 'hop' in spec(hop=0) and 'B=' in spec(B=65536) and 'L=' in spec(L=0)
    assert 'reflect' in spec(L=192) and 'shorter than one frame' in spec(L=100, pl=0, pr=0, mode=0) and 'pad_mode' in spec(mode=2)
    for x, di, do in ((None, Bp, Cp), (A, None, Cp), (A, Bp, None)):
        assert 'null' in _refused(lib, 'dsv_mel_clamp_backward', x, di, do, 100)
    assert 'n=' in _refused(lib, 'dsv_mel_clamp_backward', A, Bp, Cp, 0)
    assert 'overlaps' in _refused(lib, 'dsv_mel_clamp_backward', A, Bp, A + 40, 100)
    assert 'overlaps' in _refused(lib, 'dsv_mel_clamp_backward', A, Bp, Bp + 40, 100)


def _spectrum(n_fft, hop, L, B, seed, zero=None):
    x = SH.make_signal(L, seed=seed, batch=B)
    if zero is not None:
        x[:, zero[0]:zero[1]] = 0
    return torch.view_as_real(SH.ref_stft64(x, n_fft, hop, n_fft, False, 'reflect', (n_fft - hop) // 2)).contiguous()


@pytest.mark.parametrize('n_fft,hop,M,mag_eps,log10,zero', [(1024, 256, 80, 1e-9, False, None), (256, 64, 33, 0.0, True, (700, 1500)),
                                                            (512, 128, 128, 1e-9, False, None)])
def test_vjp_formula_equals_autograd_in_float64(n_fft, hop, M, mag_eps, log10, zero):
    S = _spectrum(n_fft, hop, 3000, 2, 7, zero)
    g = torch.Generator().manual_seed(n_fft + M)
    W = 0.02 * torch.rand(M, n_fft // 2 + 1, generator=g, dtype=torch.float64)
    cot = torch.randn(2, S.shape[2], M, generator=g, dtype=torch.float64)
    mag0 = (S[..., 0] == 0) & (S[..., 1] == 0)
    assert bool(mag0.any()) == (zero is not None)                       # the zeroed stretch gives whole frames of exact zeros
    leaf = S.clone().requires_grad_(True)
    out, mel = MH.head64(leaf, W, mag_eps, 1e-5, log10)
    want, = torch.autograd.grad(out, leaf, cot)
    got = MH.head_vjp64(S, W, cot, mel.detach(), mag_eps, 1e-5, log10)
    if mag_eps == 0.0:
        dead = mag0[..., None].expand_as(want)
        assert bool(torch.isnan(want[dead]).all()) and float(got[dead].abs().max()) == 0.0     # autograd: 0 / 0; the convention: exactly 0
        want = torch.where(dead, torch.zeros((), dtype=torch.float64), want)
        assert bool((mel.detach() < MH.f32(1e-5)).any())                   # and those frames sit below the floor
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f'head_vjp64 vs autograd {n_fft}/{M}: max |diff| {err:.3e} <= 1e-12 x max |G| {scale:.3e}')
    assert bool(torch.isfinite(got).all()) and err <= 1e-12 * scale


def test_stft_vjp_with_a_padding_amount_equals_autograd():
    """stft_vjp composes the merged transposes on the padded length with the padding's adjoint: against autograd through ref_stft64."""
    n_fft, hop, L = 256, 64, 700
    o = MH.flavour('hifigan', n_fft, hop)
    g = torch.Generator().manual_seed(3)
    x = torch.zeros(2, L, dtype=torch.float64, requires_grad=True)
    S = torch.view_as_real(SH.ref_stft64(x, n_fft, hop, n_fft, o['center'], o['pad_mode'], o['pad']))
    G = torch.randn(S.shape, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(S, x, G)
    got64, got32 = MH.stft_vjp(G, L, n_fft, hop, n_fft, o), MH.stft_vjp(G, L, n_fft, hop, n_fft, o, torch.float32)
    scale = float(want.abs().max())
    assert float((got64 - want).abs().max()) <= 1e-12 * scale and float((got32.double() - want).abs().max()) <= 1e-5 * scale


def test_python_refusals_need_no_device():
    from diffsinger_amd import HifiGanMelLoss, mel_spectrogram_loss_op, spec_logmel_op
    from diffsinger_amd.stft import logmel_op
    hp = dict(fft_size=512, hop_size=128, win_size=512, audio_num_mel_bins=80, fmin=30, fmax=12000, audio_sample_rate=24000)
    W = torch.zeros(80, 257)
    x, y, mel = torch.zeros(2, 2048), torch.zeros(2, 2048), torch.zeros(2, 16, 80)
    crit = HifiGanMelLoss(hp, mel_basis=W)
    with pytest.raises(NotImplementedError, match='target'):
        crit(x, y.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match='target'):
        crit(x, mel=mel.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match='target'):
        mel_spectrogram_loss_op(x, mel.clone().requires_grad_(True), W, n_fft=512, hop=128)
    with pytest.raises(NotImplementedError, match='mel basis'):
        mel_spectrogram_loss_op(x, mel, W.clone().requires_grad_(True), n_fft=512, hop=128)
    with pytest.raises(NotImplementedError, match='mel basis'):
        spec_logmel_op(torch.zeros(2, 257, 16, 2), W.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match='mel basis'):
        logmel_op(x.clone().requires_grad_(True), W.clone().requires_grad_(True), n_fft=512, hop=128, flavour='hifigan')
    with pytest.raises(NotImplementedError, match='mel basis'):
        HifiGanMelLoss(hp, mel_basis=W.clone().requires_grad_(True))
    for kw in (dict(lengths=[2048, 2000]), dict(return_linear=True), dict(return_frames=True)):
        with pytest.raises(NotImplementedError, match='no gradient'):
            logmel_op(x.clone().requires_grad_(True), W, n_fft=512, hop=128, flavour='hifigan', **kw)
    with pytest.raises(RuntimeError, match='no CPU path'):
        crit(x, y)
    with pytest.raises(RuntimeError, match='no CPU path'):
        crit(x, mel=mel)
    with pytest.raises(RuntimeError, match='no CPU path'):
        mel_spectrogram_loss_op(x, mel, W, n_fft=512, hop=128)
    with pytest.raises(RuntimeError, match='no CPU path'):
        spec_logmel_op(torch.zeros(2, 257, 16, 2), W)
    with pytest.raises(RuntimeError, match='no CPU path'):
        logmel_op(x.clone().requires_grad_(True), W, n_fft=512, hop=128, flavour='hifigan')
    for M in (0, 129):
        with pytest.raises(ValueError, match='mel bins'):
            spec_logmel_op(torch.zeros(2, 257, 16, 2), torch.zeros(M, 257))
        with pytest.raises(ValueError, match='mel bins'):
            mel_spectrogram_loss_op(x, torch.zeros(2, 16, M), torch.zeros(M, 257), n_fft=512, hop=128)
        with pytest.raises(ValueError, match='mel bins'):
            HifiGanMelLoss(dict(hp, audio_num_mel_bins=M))
    with pytest.raises(ValueError, match='not both'):
        crit(x, y, mel=mel)
    with pytest.raises(ValueError):
        crit(x, torch.zeros(2, 1000))
    with pytest.raises(KeyError, match='fmin'):
        HifiGanMelLoss({k: v for k, v in hp.items() if k != 'fmin'})


def test_public_names():
    import diffsinger_amd
    for name in ('HifiGanMelLoss', 'mel_spectrogram_loss_op', 'spec_logmel_op', 'hifigan_generator_losses', 'hifigan_generator_step'):
        assert name in diffsinger_amd.__all__ and callable(getattr(diffsinger_amd, name))


def test_signals_are_what_the_gpu_tests_state():
    x, y = MH.signals('loud', 8192, 2)
    share = float((x.abs() > 1).double().mean())
    print(f'loud: {100 * share:.2f} % of the samples exceed +-1')
    assert 0.02 < share < 0.12
    x, y = MH.signals('silence', 8192, 2)
    assert float(x[:, 2048:6144].abs().max()) == 0.0 and float(y[1, 2731:5461].abs().max()) == 0.0 and float(y[0].abs().min()) >= 0.0
    x, y = MH.signals('quiet', 8192, 2)
    assert float(x.abs().max()) < 1e-4
    assert np.isfinite(float(MH.ref_loss64(x, y, torch.rand(40, 129), 256, 64, 256)))
