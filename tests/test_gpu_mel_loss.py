"""GPU: the mel loss (include/dsv.h section "Mel loss", csrc/voc_mel.hpp) - the head and its vector-Jacobian product through the C ABI and
spec_logmel_op, the differentiable logmel_op, HifiGanMelLoss end to end, determinism and graph capture, one generator step, the refusals.

The yardstick rule of the STFT family (tests/stft_helpers.py, tests/mel_loss_helpers.py): the kernel and a float32 evaluation on the CPU are
fp32 sums of the same products in a different order, so the kernel's error against float64 may be 2 x the float32 evaluation's - both taken
from the DEVICE'S OWN operands (its spectrum; for gradients its saved linear mel decides the floor branch on both sides, and for the loss the
L1's signs are anchored on the device's own log-mel).  Shapes are the smallest at which the kernels can go wrong: one frame, the 32-frame
block's seams, one and 128 mel rows, a mel row tile with one row, the bin tile that holds bin n_fft / 2 alone.  Every test prints its measured
maximum beside its bound."""
import functools

import numpy as np
import pytest
import torch

from tests import hifigan_train_helpers as TH
from tests import mel_loss_helpers as MH
from tests import stft_helpers as SH

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def slaney(sr, n_fft, M, fmin, fmax):
    from diffsinger_amd.stft import mel_filterbank              # DATA: the operators take the basis from the caller
    return torch.from_numpy(mel_filterbank(sr, n_fft, M, fmin, fmax))


def within(name, got, want, yard, scale=None):
    """max |got - want| <= 2 max |yard - want| (optionally both relative to `scale`), printed"""
    want = want.double()
    err, bound = float((got.double().cpu() - want).abs().max()), 2.0 * float((yard.double() - want).abs().max())
    s = 1.0 if scale is None else scale
    print(f'{name}: max err {err / s:.3e} <= bound {bound / s:.3e} (2 x the float32 CPU evaluation){"" if scale is None else f", relative to {s:.3e}"}')
    assert bool(torch.isfinite(got).all()), f'{name}: not every element was written'
    assert err <= bound, name
    return err, bound


# ------------------------------------------------------------------------------------------------------------------------------------
# 1 / 2. the head and its vector-Jacobian product at the seams
# ------------------------------------------------------------------------------------------------------------------------------------
# (n_fft, T, M, B, spectrum, basis, mag_eps, log10)
HEAD_CASES = [(512, 1, 80, 2, 'rand', 'dense', 1e-9, False), (512, 31, 80, 2, 'stft', 'dense', 1e-9, True), (512, 32, 80, 2, 'rand', 'dense', 1e-9, False),
              (512, 33, 80, 2, 'stft', 'dense', 1e-9, False), (512, 64, 80, 2, 'rand', 'dense', 1e-9, True), (512, 65, 80, 2, 'stft', 'slaney', 1e-9, False),
              (512, 130, 80, 2, 'stft', 'dense', 1e-9, False),
              (256, 33, 1, 2, 'stft', 'dense', 1e-9, False), (256, 33, 32, 2, 'rand', 'dense', 1e-9, False), (256, 33, 33, 2, 'stft', 'dense', 0.0, True),
              (256, 33, 128, 2, 'rand', 'dense', 0.0, False),
              (2048, 65, 128, 3, 'stft', 'dense', 1e-9, False)]
FLOOR = 1e-5


@functools.lru_cache(maxsize=None)
def head_case(n_fft, T, M, B, kind, basis, mag_eps, log10):
    """-> dict of the device's spectrum, the basis, the device's outputs and the CPU evaluations, computed once per case"""
    from diffsinger_amd.stft import spec_logmel_op, stft_op
    g = torch.Generator().manual_seed(n_fft + 7 * T + M)
    hop, n_bins = n_fft // 4, n_fft // 2 + 1
    W = slaney(24000, n_fft, M, 30, 12000) if basis == 'slaney' else 0.02 * torch.rand(M, n_bins, generator=g)
    if kind == 'stft':                                                          # hifigan framing: L = T hop samples are T frames
        x, _ = MH.signals('silence', T * hop, B)
        pad = (n_fft - hop) // 2
        S = torch.view_as_real(stft_op(x.to(DEV), n_fft=n_fft, hop=hop, center=False, pad_mode='reflect', pad=pad)).contiguous()
    else:                                                                       # frames of 1e-3 .. 1e+2, imaginary parts at bins 0 and n_fft / 2 too
        scale = 10.0 ** (torch.rand(B, 1, T, 1, generator=g) * 5 - 3)
        S = (torch.randn(B, n_bins, T, 2, generator=g) * scale).to(DEV)
        assert float(S[:, 0, :, 1].abs().min()) > 0 and float(S[:, -1, :, 1].abs().min()) > 0
    assert S.shape == (B, n_bins, T, 2)
    out, mel = spec_logmel_op(S, W.to(DEV), mag_eps=mag_eps, floor=FLOOR, log10=log10, return_linear_mel=True)
    Sc = S.cpu()
    o64, m64 = MH.head64(Sc, W, mag_eps, FLOOR, log10)
    o32, m32 = MH.head32(Sc, W, mag_eps, FLOOR, log10)
    return dict(S=S, Sc=Sc, W=W, out=out, mel=mel, o64=o64, m64=m64, o32=o32, m32=m32, g=g)


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: f'{c[0]}-T{c[1]}-M{c[2]}-{c[4]}-{c[5]}')
def test_head_forward_at_the_seams(case):
    n_fft, T, M, B, kind, basis, mag_eps, log10 = case
    c = head_case(*case)
    assert c['out'].shape == c['mel'].shape == (B, T, M)
    within(f'log-mel {case}', c['out'], c['o64'], c['o32'])
    within(f'linear mel {case}', c['mel'], c['m64'], c['m32'], scale=float(c['m64'].abs().max()))
    zero = (c['Sc'].abs().amax(dim=(1, 3)) == 0)                                # [B][T]: frames of exact zeros
    if kind == 'stft' and T >= 31:
        assert bool(zero.any())
    if bool(zero.any()) and basis == 'slaney':
        want = np.float32(np.log10(np.float64(np.float32(FLOOR))) if log10 else np.log(np.float64(np.float32(FLOOR))))
        cells = c['out'].cpu()[zero]
        print(f'{int(zero.sum())} frames of exact zeros: every cell is float32(log(floor)) = {want!r}')
        assert bool((cells == float(want)).all())


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: f'{c[0]}-T{c[1]}-M{c[2]}-{c[4]}-{c[5]}')
def test_head_vjp(case):
    from diffsinger_amd import _lib
    from diffsinger_amd.stft import spec_logmel_op
    n_fft, T, M, B, kind, basis, mag_eps, log10 = case
    c = head_case(*case)
    S, W = c['S'], c['W']
    cot = torch.randn(B, T, M, generator=torch.Generator().manual_seed(T + M))
    leaf = S.clone().requires_grad_(True)
    out, mel = spec_logmel_op(leaf, W.to(DEV), mag_eps=mag_eps, floor=FLOOR, log10=log10, return_linear_mel=True)
    assert torch.equal(out, c['out']) and torch.equal(mel, c['mel']) and not mel.requires_grad
    G, = torch.autograd.grad(out, leaf, cot.to(DEV))
    direct = torch.full(S.shape, NAN, device=DEV)
    Wd, gd = W.to(DEV).contiguous(), cot.to(DEV).contiguous()
    _lib.call('dsv_mel_head_backward', S.device, S.data_ptr(), Wd.data_ptr(), gd.data_ptr(), c['mel'].data_ptr(), direct.data_ptr(), B, T, n_fft, M,
              mag_eps, FLOOR, 1 if log10 else 0)
    assert torch.equal(G, direct), 'autograd through spec_logmel_op is not the one launch of the C ABI'
    mel_dev = c['mel'].cpu()
    want = MH.head_vjp64(c['Sc'], W, cot, mel_dev, mag_eps, FLOOR, log10)
    yard = MH.head_vjp32(c['Sc'], W, cot, mel_dev, mag_eps, FLOOR, log10)
    within(f'G {case} (max |G| {float(want.abs().max()):.3e})', G, want, yard)
    Gc = G.cpu()
    floored = (mel_dev < MH.f32(FLOOR)).all(dim=2)                              # [B][T]: frames whose cells are all on the floor
    if bool(floored.any()):
        dead = floored[:, None, :, None].expand_as(Gc)
        print(f'{int(floored.sum())} fully floored frames: exact zeros in every bin')
        assert float(Gc[dead].abs().max()) == 0.0
    if kind == 'stft' and (basis == 'slaney' or mag_eps == 0.0):               # the silent stretch: sqrt(mag_eps) under a unit-area basis, or 0
        assert bool(floored.any())
    if mag_eps == 0.0:
        mag0 = (c['Sc'][..., 0] == 0) & (c['Sc'][..., 1] == 0)
        assert bool(mag0.any()) == (kind == 'stft')
        if bool(mag0.any()):
            assert float(Gc[mag0].abs().max()) == 0.0
    if kind == 'rand':                                                          # live cells: the gradient is really there
        assert float(Gc.abs().max()) > 0 and float(Gc[:, 0, :, 1].abs().max()) > 0 and float(Gc[:, -1, :, 1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. differentiable logmel_op
# ------------------------------------------------------------------------------------------------------------------------------------
def lengths_of(n_fft, hop):
    return ((8192, 2), (n_fft + 3 * hop + 17, 1))


def chain_operands(x, W, n_fft, hop, win, o):
    """the device's own spectrum and saved linear mel of the chain, through the public operators -> (S [B][n_bins][T][2], log-mel, mel) on the CPU"""
    from diffsinger_amd.stft import spec_logmel_op, stft_op
    xd = x.to(DEV)
    xd = xd.clamp(-1.0, 1.0) if o['clamp'] else xd
    S = torch.view_as_real(stft_op(xd, n_fft=n_fft, hop=hop, win_length=win, center=o['center'], pad_mode=o['pad_mode'], pad=o['pad'])).contiguous()
    out, mel = spec_logmel_op(S, W.to(DEV), mag_eps=o['mag_eps'], floor=o['floor'], log10=o['log10'], return_linear_mel=True)
    return S.cpu(), out, mel.cpu()


def chain_vjps(S, W, cot, mel_dev, x, L, n_fft, hop, win, o):
    """(float64, float32) of clampmask . stft_vjp(head_vjp(S_dev, ...)): the chain's gradient restated from the device's spectrum"""
    mask = MH.clamp_mask(x, o)
    want = mask * MH.stft_vjp(MH.head_vjp64(S, W, cot, mel_dev, o['mag_eps'], o['floor'], o['log10']), L, n_fft, hop, win, o)
    yard = mask * MH.stft_vjp(MH.head_vjp32(S, W, cot, mel_dev, o['mag_eps'], o['floor'], o['log10']), L, n_fft, hop, win, o, torch.float32).double()
    return want, yard


LOGMEL_CASES = [(g, i, 'hifigan', s) for g in range(4) for i in range(2) for s in ('near', 'loud', 'silence')] + [(0, 0, 'pwg', 'near'), (3, 1, 'pwg', 'near')]


@pytest.mark.parametrize('geo,which,flavour,sig', LOGMEL_CASES)
def test_differentiable_logmel(geo, which, flavour, sig):
    from diffsinger_amd.stft import logmel_op
    n_fft, hop, win, sr, M, fmin, fmax = MH.GEOMETRIES[geo]
    L, B = lengths_of(n_fft, hop)[which]
    o = MH.flavour(flavour, n_fft, hop)
    W = slaney(sr, n_fft, M, fmin, fmax)
    x, _ = MH.signals(sig, L, B)
    one = (0, L // 2)
    if sig == 'loud':
        x[one] = 1.0                                                            # exactly on the clamp's edge: the gradient passes
        over = x.abs() > 1
        print(f'loud: {100 * float(over.double().mean()):.2f} % of the samples exceed +-1')
        assert bool(over.any())
    Wd = W.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out_d = logmel_op(xg, Wd, n_fft=n_fft, hop=hop, win_length=win, flavour=flavour)
    out_f = logmel_op(x.to(DEV), Wd, n_fft=n_fft, hop=hop, win_length=win, flavour=flavour)
    assert out_d.grad_fn is not None and out_f.grad_fn is None
    ref = SH.ref_logmel64(x, W, flavour, n_fft, hop, win)[0]
    y32 = SH.yardstick32(x, n_fft, hop, win, basis=W, flavour=flavour)[0]
    within(f'values, differentiable path {n_fft}/{hop} L={L} {flavour} {sig}', out_d.detach(), ref, y32)
    within(f'values, fused path          {n_fft}/{hop} L={L} {flavour} {sig}', out_f, ref, y32)
    cot = torch.randn(ref.shape, generator=torch.Generator().manual_seed(geo * 10 + which))
    dx, = torch.autograd.grad(out_d, xg, cot.to(DEV))
    S, out_s, mel_dev = chain_operands(x, W, n_fft, hop, win, o)
    assert torch.equal(out_s, out_d.detach()), 'the chain is not dsv_mel_spectrum -> dsv_mel_head on the bits of stft_op'
    want, yard = chain_vjps(S, W, cot, mel_dev, x, L, n_fft, hop, win, o)
    within(f'dx {n_fft}/{hop} L={L} {flavour} {sig} (max |dx| {float(want.abs().max()):.3e})', dx, want, yard)
    if sig == 'loud':
        dxc = dx.cpu()
        assert float(dxc[over].abs().max()) == 0.0 and float(dxc[one].abs()) > 0.0
        print(f'{int(over.sum())} clamped samples carry exactly 0; the sample at exactly 1.0 carries {float(dxc[one]):.3e}')


def test_logmel_without_grad_is_the_fused_launch(monkeypatch):
    from diffsinger_amd import _lib
    from diffsinger_amd.stft import bases, logmel_op
    n_fft, hop, win, sr, M, fmin, fmax = MH.GEOMETRIES[1]
    W = slaney(sr, n_fft, M, fmin, fmax).to(DEV)
    x = MH.signals('loud', 4096, 2)[0].to(DEV)
    base = logmel_op(x, W, n_fft=n_fft, hop=hop, win_length=win, flavour='hifigan')
    xg = x.clone().requires_grad_(True)
    out_g = logmel_op(xg, W, n_fft=n_fft, hop=hop, win_length=win, flavour='hifigan')       # warm-up of the chain (adjoint basis)
    torch.autograd.grad(out_g.sum(), xg)
    calls, real = [], _lib.check

    def spy(rc, what=''):
        calls.append(what)
        return real(rc, what)
    monkeypatch.setattr(_lib, 'check', spy)
    with torch.no_grad():
        quiet = logmel_op(xg, W, n_fft=n_fft, hop=hop, win_length=win, flavour='hifigan')
    assert calls == ['dsv_logmel'] and torch.equal(quiet, base) and quiet.grad_fn is None
    del calls[:]
    assert torch.equal(logmel_op(x, W, n_fft=n_fft, hop=hop, win_length=win, flavour='hifigan'), base) and calls == ['dsv_logmel']
    # the same bits as the C ABI's fused launch called directly
    direct = torch.full(base.shape, NAN, device=DEV)
    fwd, _ = bases(DEV, n_fft, win)
    pad = (n_fft - hop) // 2
    _lib.call('dsv_logmel', x.device, x.data_ptr(), None, fwd.data_ptr(), W.data_ptr(), direct.data_ptr(), None, None, 2, 4096, n_fft, hop, pad, pad, 1, 1, M,
              1e-9, 1e-5, 0)
    assert torch.equal(direct, base)
    for flavour, back in (('hifigan', ['dsv_mel_head_backward', 'dsv_stft_adjoint', 'dsv_mel_clamp_backward']), ('pwg', ['dsv_mel_head_backward', 'dsv_stft_adjoint'])):
        del calls[:]
        out = logmel_op(xg, W, n_fft=n_fft, hop=hop, win_length=win, flavour=flavour)
        assert calls == ['dsv_mel_spectrum', 'dsv_mel_head'], calls
        del calls[:]
        torch.autograd.grad(out.sum(), xg)
        assert calls == back, calls
    print('logmel_op: one dsv_logmel launch without a gradient (the bits of the direct call); with one, spectrum -> head and head backward -> adjoint [-> clamp mask]')


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the loss end to end
# ------------------------------------------------------------------------------------------------------------------------------------
def criterion(geo):
    from diffsinger_amd import HifiGanMelLoss
    n_fft, hop, win, sr, M, fmin, fmax = MH.GEOMETRIES[geo]
    return HifiGanMelLoss(dict(fft_size=n_fft, hop_size=hop, win_size=win, audio_num_mel_bins=M, fmin=fmin, fmax=fmax, audio_sample_rate=sr)).to(DEV)


@pytest.mark.parametrize('sig', ['near', 'far', 'silence', 'quiet'])
@pytest.mark.parametrize('geo,which', [(g, i) for g in range(4) for i in range(2)])
def test_loss_end_to_end(geo, which, sig):
    n_fft, hop, win, sr, M, fmin, fmax = MH.GEOMETRIES[geo]
    L, B = lengths_of(n_fft, hop)[which]
    o = MH.flavour('hifigan', n_fft, hop)
    W = slaney(sr, n_fft, M, fmin, fmax)
    crit = criterion(geo)
    x, y = MH.signals(sig, L, B)
    xg, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    loss = crit(xg, yd)
    assert loss.dim() == 0
    dx, = torch.autograd.grad(loss, xg)
    x64 = x.double().requires_grad_(True)
    ref = MH.ref_loss64(x64, y, W, n_fft, hop, win)
    dref, = torch.autograd.grad(ref, x64)
    rel = abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach())
    tgt = crit.analyse(yd)
    floor_share = float((tgt <= np.log(np.float32(1e-5)) + 1e-6).double().mean())
    print(f'loss {n_fft}/{hop} L={L} {sig}: {float(loss.detach()):.6f}, relative error {rel:.3e} <= 1e-5; {100 * floor_share:.0f} % of the target cells on the floor')
    assert rel <= 1e-5
    # the gradient: the L1's signs anchored on the device's own log-mel
    S, out_s, mel_dev = chain_operands(x, W, n_fft, hop, win, o)
    assert torch.equal(out_s, crit.analyse(xg.detach()))
    cot = torch.sign(out_s.cpu().double() - tgt.cpu().double()) / out_s.numel()
    want, yard = chain_vjps(S, W, cot, mel_dev, x, L, n_fft, hop, win, o)
    within(f'dx {n_fft}/{hop} L={L} {sig} (max |dx| {float(want.abs().max()):.3e})', dx, want, yard)
    print(f'   distance to the float64 gradient from the waveforms: {float((dx.cpu().double() - dref).abs().max() / dref.abs().max()):.3e} of max |dx| (printed only)')
    # a ready log-mel target is the waveform target path, bit for bit
    x2 = x.to(DEV).requires_grad_(True)
    loss2 = crit(x2, mel=tgt)
    dx2, = torch.autograd.grad(loss2, x2)
    assert torch.equal(loss2, loss) and torch.equal(dx2, dx)
    # loss(x, x) is exactly 0, and so is its gradient
    x3 = x.to(DEV).requires_grad_(True)
    zero = crit(x3[:, None], x.to(DEV)[:, None])                               # [B][1][L] is accepted
    dz, = torch.autograd.grad(zero, x3)
    assert float(zero.detach()) == 0.0 and float(dz.abs().max()) == 0.0


def test_mel_spectrogram_loss_op_is_the_module():
    from diffsinger_amd import mel_spectrogram_loss_op
    n_fft, hop, win, sr, M, fmin, fmax = MH.GEOMETRIES[3]
    crit = criterion(3)
    x, y = MH.signals('far', 2048, 2)
    tgt = crit.analyse(y.to(DEV))
    xa, xb = x.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    a = mel_spectrogram_loss_op(xa, tgt, crit.basis_on(DEV), n_fft=n_fft, hop=hop, win_length=win)
    b = crit(xb, mel=tgt)
    assert torch.equal(a, b) and torch.equal(torch.autograd.grad(a, xa)[0], torch.autograd.grad(b, xb)[0])
    with pytest.raises(ValueError, match='frames'):
        mel_spectrogram_loss_op(xa, tgt[:, :-1], crit.basis_on(DEV), n_fft=n_fft, hop=hop, win_length=win)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. determinism and capture
# ------------------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_graph_capture():
    crit = criterion(0)
    x, y = MH.signals('near', 8192, 2)
    x2, _ = MH.signals('silence', 8192, 2)
    y = y.to(DEV)

    def run(wav):
        xg = wav.to(DEV).requires_grad_(True)
        loss = crit(xg, y)
        dx, = torch.autograd.grad(loss, xg)
        return loss.detach().clone(), dx.clone()

    a, b = run(x), run(x)
    assert all(torch.equal(p, q) for p, q in zip(a, b))                        # two eager calls: bitwise equal, value and dx
    eager2 = run(x2)                                                          # (also the warm-up: every basis is built)
    static = x.to(DEV).clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a host sync or a .item() inside would fail the capture itself
        loss = crit(static, y)
        dx, = torch.autograd.grad(loss, static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, a[0]) and torch.equal(dx, a[1])
    with torch.no_grad():
        static.copy_(x2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager2[0]) and torch.equal(dx, eager2[1])
    print('HifiGanMelLoss forward + backward: one captured graph on one stream, replays carry the bits of the eager calls')


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. one generator step
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['nsf', 'plain'])
def test_generator_step(case):
    from diffsinger_amd import HifiGanMelLoss, hifigan_generator_losses, hifigan_generator_step
    from diffsinger_amd.vocoder import HifiGanGenerator
    from tests.voc_helpers import draws_like_reference
    fx = TH.fixture(case)
    h = fx['h']
    gen = HifiGanGenerator(h)
    gen.load_state_dict(fx['state'], strict=True)
    gen = gen.to(DEV)
    B, T, hop = 2, 40, TH.hop_of(h)
    assert hop == 64
    crit = HifiGanMelLoss(dict(fft_size=256, hop_size=hop, win_size=256, audio_num_mel_bins=40, fmin=0, fmax=12000, audio_sample_rate=24000)).to(DEV)
    batch = dict(x=torch.randn(B, 80, T, generator=torch.Generator().manual_seed(71)).to(DEV),
                 y=MH.signals('near', T * hop, B)[1][:, None].to(DEV))
    if case == 'nsf':
        ri, nz = draws_like_reference(72, B, T * hop)
        batch.update(f0=(220.0 + torch.zeros(B, T)).to(DEV), rand_ini=ri.to(DEV), noise=nz.to(DEV))
    hp = dict(lambda_mel=45.0)
    out = hifigan_generator_step(gen, crit, batch, hp)
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in gen.named_parameters()}
    assert sorted(k for k, g in grads.items() if g is None) == sorted(fx['none_keys'])
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)
    norm = float(out['gen_grad_norm'])
    print(f'{case}: mel {float(out["gen_mel"]):.5f}, total {float(out["gen_total"]):.4f}, gradient norm {norm:.4e}')
    assert np.isfinite(norm) and norm > 0 and float(out['gen_total']) == float(np.float32(45.0) * out['gen_mel'].cpu().numpy())
    # the cotangent trick: a second step driven by (y_hat . dL/dy_hat).sum() gives the same parameter gradients, bit for bit
    kw = dict(rand_ini=batch.get('rand_ini'), noise=batch.get('noise'))
    losses, y_hat = hifigan_generator_losses(gen, crit, batch['x'], batch.get('f0'), batch['y'], lambda_mel=45.0, **kw)
    assert torch.equal(losses['total'].detach(), out['gen_total'])
    leaf = y_hat.detach().clone().requires_grad_(True)
    cot, = torch.autograd.grad(45.0 * crit(leaf, batch['y']), leaf)
    for p in gen.parameters():
        p.grad = None
    y2 = gen.forward_train(batch['x'], batch.get('f0'), **kw)
    (y2 * cot).sum().backward()
    assert torch.equal(y2, y_hat)
    assert all(torch.equal(p.grad, grads[k]) for k, p in gen.named_parameters() if grads[k] is not None)
    # lambda_mel doubled: the total doubles exactly
    doubled, _ = hifigan_generator_losses(gen, crit, batch['x'], batch.get('f0'), batch['y'], lambda_mel=90.0, **kw)
    assert torch.equal(doubled['total'].detach(), 2.0 * losses['total'].detach()) and torch.equal(doubled['mel'], losses['mel'])
    # clipping only when hp carries generator_grad_norm; the norm returned is the one before clipping
    clipped = hifigan_generator_step(gen, crit, batch, dict(hp, generator_grad_norm=1e-3))
    after = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in gen.parameters() if p.grad is not None])))
    assert torch.equal(clipped['gen_grad_norm'], out['gen_grad_norm']) and after <= 1e-3 * (1 + 1e-4)
    # a small SGD step lowers the loss on the same batch and source draws
    opt = torch.optim.SGD([p for p in gen.parameters() if p.requires_grad], lr=1e-3 / norm)
    first = hifigan_generator_step(gen, crit, batch, hp, opt_g=opt)
    with torch.no_grad():
        second, _ = hifigan_generator_losses(gen, crit, batch['x'], batch.get('f0'), batch['y'], lambda_mel=45.0, **kw)
    print(f'{case}: mel loss {float(first["gen_mel"]):.6f} -> {float(second["mel"]):.6f} after one SGD step of length 1e-3')
    assert torch.equal(first['gen_mel'], out['gen_mel']) and float(second['mel']) < float(first['gen_mel'])


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. ABI refusals through real pointers
# ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    from diffsinger_amd import _lib
    from diffsinger_amd.stft import bases
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    B, T, n_fft, M = 2, 33, 512, 80
    big = torch.zeros(B * 257 * T * 2 + B * T * M, device=DEV)                    # one allocation: overlaps can be built on purpose
    S, tail = big[:B * 257 * T * 2], big[B * 257 * T * 2:]
    W, out, mel, g, G = torch.zeros(M, 257, device=DEV), torch.zeros(B, T, M, device=DEV), torch.ones(B, T, M, device=DEV), \
        torch.zeros(B, T, M, device=DEV), torch.zeros(B, 257, T, 2, device=DEV)
    ok = (B, T, n_fft, M, 1e-9, 1e-5, 0)
    p = lambda t: t.data_ptr()                                                    # noqa: E731
    assert lib.dsv_mel_head(p(S), p(W), p(out), p(mel), *ok, s) == 0
    assert lib.dsv_mel_head_backward(p(S), p(W), p(g), p(mel), p(G), *ok, s) == 0
    assert lib.dsv_mel_head(p(S), p(W), p(tail), p(mel), *ok, s) == 0             # adjacent is not overlapping
    for args, msg in (((p(S), p(W), p(S) + 8, p(mel)), b'overlaps'), ((p(S), p(W), p(out), p(tail) - 4), b'overlaps'), ((p(S), p(W), p(out), p(out)), b'overlaps'),
                      ((p(S), p(W), p(W), p(mel)), b'overlaps'), ((p(S) + 4, p(W), p(out), p(mel)), b'aligned'), ((None, p(W), p(out), p(mel)), b'null')):
        assert lib.dsv_mel_head(*args, *ok, s) == -1 and msg in lib.dsd_last_error() and b'dsv_mel_head:' in lib.dsd_last_error(), (msg, lib.dsd_last_error())
    for Gp in (p(S), p(S) + 8, p(W), p(g), p(mel)):
        assert lib.dsv_mel_head_backward(p(S), p(W), p(g), p(mel), Gp, *ok, s) == -1 and b'overlaps' in lib.dsd_last_error()
    for bad, msg in (((B, T, 384, M, 1e-9, 1e-5, 0), b'n_fft=384'), ((B, T, n_fft, 0, 1e-9, 1e-5, 0), b'M=0'), ((B, T, n_fft, 129, 1e-9, 1e-5, 0), b'M=129'),
                     ((B, 0, n_fft, M, 1e-9, 1e-5, 0), b'T=0'), ((0, T, n_fft, M, 1e-9, 1e-5, 0), b'B=0'), ((70000, T, n_fft, M, 1e-9, 1e-5, 0), b'B=70000'),
                     ((B, T, n_fft, M, -1.0, 1e-5, 0), b'mag_eps'), ((B, T, n_fft, M, 1e-9, 0.0, 0), b'floor'), ((B, T, n_fft, M, 1e-9, float('inf'), 0), b'finite')):
        assert lib.dsv_mel_head(p(S), p(W), p(out), p(mel), *bad, s) == -1 and msg in lib.dsd_last_error(), (msg, lib.dsd_last_error())
        assert lib.dsv_mel_head_backward(p(S), p(W), p(g), p(mel), p(G), *bad, s) == -1 and msg in lib.dsd_last_error(), (msg, lib.dsd_last_error())
    fwd, _ = bases(DEV, n_fft, n_fft)
    wav, spec = torch.zeros(1, 4096, device=DEV), torch.zeros(1, 257, 32, 2, device=DEV)
    assert lib.dsv_mel_spectrum(p(wav), p(fwd), p(spec), 1, 4096, n_fft, 128, 192, 192, 1, 1, s) == 0
    for args, msg in (((1, 4096, 500, 128, 192, 192, 1, 1), b'n_fft=500'), ((1, 100, n_fft, 128, 192, 192, 1, 1), b'reflect padding'),
                      ((1, 4096, n_fft, 0, 192, 192, 1, 1), b'hop=0'), ((1, 4096, n_fft, 128, 192, 192, 3, 1), b'pad_mode')):
        assert lib.dsv_mel_spectrum(p(wav), p(fwd), p(spec), *args, s) == -1 and msg in lib.dsd_last_error() and b'dsv_mel_spectrum' in lib.dsd_last_error()
    assert lib.dsv_mel_spectrum(p(wav), p(fwd), None, 1, 4096, n_fft, 128, 192, 192, 1, 1, s) == -1 and b'null' in lib.dsd_last_error()
    # the clamp mask: in place is allowed, NaN and out-of-range samples give 0, +-1 pass
    x = torch.tensor([0.5, 1.0, -1.0, 1.0000001, -1.5, NAN, 0.0], device=DEV)
    d = torch.arange(1.0, 8.0, device=DEV)
    o = torch.full((7,), NAN, device=DEV)
    assert lib.dsv_mel_clamp_backward(p(x), p(d), p(o), 7, s) == 0 and lib.dsv_mel_clamp_backward(p(x), p(d), p(d), 7, s) == 0
    assert lib.dsv_mel_clamp_backward(p(x), p(d), p(x), 7, s) == -1 and b'overlaps' in lib.dsd_last_error()
    assert lib.dsv_mel_clamp_backward(p(x), p(d), p(d) + 4, 6, s) == -1 and b'overlaps' in lib.dsd_last_error()
    assert lib.dsv_mel_clamp_backward(p(x), p(d), p(o), 0, s) == -1 and b'n=0' in lib.dsd_last_error()
    torch.cuda.synchronize()
    assert o.cpu().tolist() == [1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 7.0] and torch.equal(o, d)
    assert float(out.abs().max()) > 0 and bool(torch.isfinite(out).all()) and float(G.abs().max()) == 0.0
