"""GPU: the STFT loss (include/dsv.h section "STFT loss", csrc/voc_stft_loss.hpp) through diffsinger_amd.stft_loss, against the float64
restatements of tests/stft_loss_helpers.py (torch.stft, autograd and numpy on the CPU).

Bounds, none of them taken from what the kernels give:
  adjoint STFT      2 x the error of the same transpose as a float32 torch.matmul on the CPU (adjoint_matmul) against the float64 VJP on the
                    test's own cotangent - the family's yardstick rule (tests/test_gpu_stft.py): both are fp32 sums of the same products.
                    <stft_op(x), G2> = <x, adjoint(G2)> to 1e-5 of the inner product, with G2 = S64(x) + N(0, 1): the Gaussian cotangent alone
                    makes the inner product cancel (see the comment in the test), so the transpose identity is held on one that does not.
  loss from spectra anchored on the DEVICE'S spectra, so the conditioning of the analysis drops out: with u = 2^-24
                    |sc - sc64| <= 16 u kappa sc, kappa = sum |ym - xm| (xm + ym) / sum (ym - xm)^2;  |mag - mag64| <= 16 u (1 + mean(|ln xm| + |ln ym|));
                    |G - G64| <= [16 u c + jumps] |(re, im)| element-wise (spectral64: c_sc = (|ym - xm| + xm + ym) / (xm S1 S2), c_mag = 1 / (n P),
                    the full jump of a branch only where float32 rounding can flip it).  16 = about six float32 operations (one division, one
                    square root) at <= 2.5 ulp each: a condition, not a measurement.  Clamped elements: exactly 0.
  end to end        values 1e-5 relative against float64 from the waveforms and against the reference module's fixture (float32 CPU
                    restatements sit at <= 1.1e-6; symmetric instead of periodic Hann moves sc by 2.5e-5, zero instead of reflect padding by
                    >= 3.7e-3).  Gradient per sample: 2 x the adjoint yardstick + the element-wise budget of G pushed through |A|^T, against
                    sum_r VJP64_r(G64_r(device spectra)) / R.  The distance to the float64 gradient FROM THE WAVEFORMS is printed only: 1 / P
                    amplifies the forward's own float32 error (CPU float32 is 1.3e-3 of max |dx| off on 'near').
Every test prints its measured maximum next to its bound."""
import os

import numpy as np
import pytest
import torch

from diffsinger_amd import MultiResolutionSTFTLoss, STFTLoss, _lib, spectral_loss_op, stft_adjoint_op
from diffsinger_amd import stft as ST
from tests import stft_helpers as SH
from tests import stft_loss_helpers as LH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = LH.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stft_loss_ref.npz')


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the adjoint is the transpose
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_fft,hop,win', [(512, 128, 512), (1024, 256, 800), (2048, 240, 1200), (256, 64, 256)])
def test_adjoint_is_the_transpose(n_fft, hop, win):
    worst = 0.0
    for L in (n_fft // 2 + 1, 9000):
        x = SH.make_signal(L, seed=L + n_fft, batch=2)
        for mode in ('constant', 'reflect'):
            for center in (True, False):
                if not center and L < n_fft:
                    continue                                                 # shorter than a frame: only the centred forms have frames
                kw = dict(n_fft=n_fft, hop=hop, win_length=win, center=center, pad_mode=mode)
                T = ST.n_frames(L, n_fft, hop, *ST._pads(n_fft, center, None))
                G = torch.randn(2, n_fft // 2 + 1, T, 2, generator=torch.Generator().manual_seed(T))
                want = LH.vjp64(G, L, n_fft, hop, win, center, mode)
                yard = float((LH.adjoint_matmul(G, L, n_fft, hop, win, center, mode).double() - want).abs().max())
                got = stft_adjoint_op(G.to(DEV), L, **kw)
                assert got.shape == (2, L) and got.dtype == torch.float32
                err = float((got.cpu().double() - want).abs().max())
                worst = max(worst, err / yard)
                # <S(x), G2> = <x, S^T(G2)> with the device's own forward, summed in float64, to 1e-5 of the inner product itself.  The cotangent of
                # this check is G2 = S64(x) + G, not the Gaussian G alone: <S, G> of a Gaussian G is a sum of ~1e5 signed products that cancels to
                # between 1e-5 and 0.1 of sum |S G| (a float32 CPU transform already misses 1e-5 of it by up to 56 x), so a bound relative to it
                # says nothing and one relative to sum |S G| cannot fail.  <S, S64 + G> = |S|^2 + <S, G> does not cancel: a scale error of 1e-4 in
                # either operator, or x[u] a[u] of a few dropped samples (each ~1 / L of the sum), moves it by more than the bound.
                S = torch.view_as_real(ST.stft_op(x.to(DEV), **kw)).cpu().double()
                G2 = (torch.view_as_real(SH.ref_stft64(x, n_fft, hop, win, center, mode)) + G.double()).float()
                a2 = stft_adjoint_op(G2.to(DEV), L, **kw).cpu().double()
                lhs, rhs = float((S * G2.double()).sum()), float((x.double() * a2).sum())
                rel = abs(lhs - rhs) / abs(lhs)
                print(f'adjoint {n_fft}/{hop}/{win} L={L} {mode} center={int(center)}: {T} frames, max-abs err {err:.3e}, CPU fp32 yardstick {yard:.3e} '
                      f'(max |dx| {float(want.abs().max()):.1f}); <Sx, G2> {lhs:.8e} vs <x, S^T G2> {rhs:.8e}: rel {rel:.2e} (bound 1e-5)')
                assert err <= 2 * yard, (L, mode, center, err, yard)
                assert rel <= 1e-5, (L, mode, center, lhs, rhs)
                # the complex form, and autograd through stft_op, are the same launch
                assert torch.equal(stft_adjoint_op(torch.view_as_complex(G.to(DEV)), L, **kw), got)
                xg = x.to(DEV).requires_grad_(True)
                Sg = ST.stft_op(xg, **kw)
                assert Sg.requires_grad and Sg.dtype == torch.complex64
                dx, = torch.autograd.grad(torch.view_as_real(Sg), xg, G.to(DEV))
                assert torch.equal(dx, got)
    print(f'adjoint {n_fft}/{hop}/{win}: worst err / yardstick {worst:.2f}')


def test_stft_op_gradient_rules():
    x = SH.make_signal(4000, seed=2, batch=2).to(DEV)
    kw = dict(n_fft=512, hop=128)
    plain = ST.stft_op(x, **kw)
    xg = x.clone().requires_grad_(True)
    S, fc = ST.stft_op(xg, return_frames=True, **kw)
    assert not plain.requires_grad and S.requires_grad
    assert torch.equal(torch.view_as_real(S.detach()), torch.view_as_real(plain)) and fc.cpu().tolist() == [32, 32]       # the same forward launch
    with torch.no_grad():
        assert not ST.stft_op(xg, **kw).requires_grad
    with pytest.raises(NotImplementedError, match='no gradient'):
        ST.stft_op(xg, subtract=0.1, **kw)
    with pytest.raises(NotImplementedError, match='no gradient'):
        ST.stft_op(xg, lengths=torch.tensor([4000, 3000]), **kw)
    # a 1-D waveform and |S|^2 summed: d/dx sum |S|^2 = 2 S^T S x
    v = SH.make_signal(3000, seed=9)
    vg = v.to(DEV).requires_grad_(True)
    P = ST.stft_op(vg, pad_mode='reflect', **kw)
    (P.real ** 2 + P.imag ** 2).sum().backward()
    v64 = v.double().requires_grad_(True)
    R = SH.ref_stft64(v64, 512, 128, 512, True, 'reflect')
    (R.real ** 2 + R.imag ** 2).sum().backward()
    err = float((vg.grad.cpu().double() - v64.grad).abs().max())
    scale = float(v64.grad.abs().max())
    print(f'd sum |S|^2 / dx through stft_op: max-abs err {err:.3e} of max {scale:.3e} (bound 2e-5 relative, the project\'s waveform tolerance)')
    assert vg.grad.shape == (3000,) and err <= 2e-5 * scale


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the loss from spectra
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['near', 'silence'])
def test_loss_from_the_devices_spectra(case):
    x, y = LH.signals(case)
    for n_fft, hop, win in LH.RESOLUTIONS:
        kw = dict(n_fft=n_fft, hop=hop, win_length=win, center=True, pad_mode='reflect')
        X = ST.stft_op(x.to(DEV), **kw).requires_grad_(True)
        Y = ST.stft_op(y.to(DEV), **kw)
        out = spectral_loss_op(X, Y)
        assert out.shape == (2,) and out.dtype == torch.float32 and out.requires_grad
        Xr, Yr = torch.view_as_real(X.detach()).cpu().numpy(), torch.view_as_real(Y).cpu().numpy()
        ref = LH.spectral64(Xr, Yr)
        sc, mag = float(out[0].detach()), float(out[1].detach())
        b_sc, b_mag = 16 * U * ref['kappa'] * ref['sc'], 16 * U * (1 + ref['mean_logs'])
        print(f"{case} {n_fft}/{hop}/{win}: {Xr.shape[2]} frames, {ref['n_clamped']} clamped, {ref['n_flippable']} flippable; sc {sc:.8f} err {abs(sc - ref['sc']):.2e} "
              f"(bound {b_sc:.2e}, kappa {ref['kappa']:.1f}); mag {mag:.8f} err {abs(mag - ref['mag']):.2e} (bound {b_mag:.2e})")
        assert abs(sc - ref['sc']) <= b_sc and abs(mag - ref['mag']) <= b_mag
        for g_sc, g_mag in ((1.0, 0.0), (0.0, 1.0), (0.75, -1.5)):
            G, = torch.autograd.grad(out, X, torch.tensor([g_sc, g_mag], device=DEV), retain_graph=True)
            assert G.dtype == torch.complex64 and G.shape == X.shape
            G = torch.view_as_real(G).cpu().numpy().astype(np.float64)
            r = LH.spectral64(Xr, Yr, g_sc, g_mag)
            err, budget = np.abs(G - r['G']), r['tol'][..., None] * np.abs(Xr.astype(np.float64))
            used = (err[budget > 0] / budget[budget > 0]).max()
            print(f"   g = ({g_sc}, {g_mag}): max |G - G64| = {err.max() / np.abs(r['G']).max():.2e} of max |G64| = {np.abs(r['G']).max():.3e}; the worst element "
                  f"uses {used:.3f} of its own budget (<= 1)")
            assert (err <= budget).all()
            assert not G[r['clamped']].any()                                  # where the clamp is active: exactly 0
        if case == 'silence':
            assert ref['n_clamped'] >= 20000
    # silence against silence, and a spectrum against itself: 0, not 0 / 0
    Z = torch.zeros(1, 129, 40, dtype=torch.complex64, device=DEV, requires_grad=True)
    out = spectral_loss_op(Z, Z.detach())
    G, = torch.autograd.grad(out.sum(), Z)
    assert out.cpu().tolist() == [0.0, 0.0] and not torch.view_as_real(G).any()
    Xs = ST.stft_op(x.to(DEV), n_fft=256, hop=64).requires_grad_(True)
    out = spectral_loss_op(Xs, Xs.detach())
    G, = torch.autograd.grad(out.sum(), Xs)
    assert out.cpu().tolist() == [0.0, 0.0] and not torch.view_as_real(G).any()
    # the float [..][2] layout is the same launch
    a = spectral_loss_op(torch.view_as_real(X.detach()), torch.view_as_real(Y))
    assert torch.equal(a, spectral_loss_op(X.detach(), Y))


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------------------------------------------
def _device_run(crit, x, y):
    xg = x.to(DEV).requires_grad_(True)
    sc, mag = crit(xg, y.to(DEV))
    assert sc.dim() == mag.dim() == 0 and sc.dtype == mag.dtype == torch.float32
    d_sc, = torch.autograd.grad(sc, xg, retain_graph=True)
    d_mag, = torch.autograd.grad(mag, xg)
    return sc.detach(), mag.detach(), d_sc, d_mag


@pytest.mark.parametrize('case', ['near', 'silence', 'short', 'odd'])
def test_multi_resolution_loss_end_to_end(case):
    x, y = LH.signals(case)
    res = LH.resolutions_of(case)
    crit = MultiResolutionSTFTLoss(*zip(*res))
    sc, mag, d_sc, d_mag = _device_run(crit, x, y)
    (sc64, mag64), w_sc, w_mag = LH.grads_of(LH.ref_loss64, x.double(), y.double(), res)
    sc32, mag32 = LH.ref_loss32(x, y, res)
    for name, got, want, cpu32 in (('sc', float(sc), float(sc64), float(sc32)), ('mag', float(mag), float(mag64), float(mag32))):
        print(f'{case} {name}: device {got:.9f}, float64 {want:.9f}: rel {abs(got - want) / want:.2e} (bound 1e-5; float32 CPU restatement {abs(cpu32 - want) / want:.2e})')
        assert abs(got - want) <= 1e-5 * want
    if len(res) == 1:                                                        # STFTLoss is the one-resolution form of the same path
        s1, m1, _, _ = _device_run(STFTLoss(*res[0]), x, y)
        assert torch.equal(s1, sc) and torch.equal(m1, mag)
    # the gradient, anchored on the device's own spectra
    B, L = x.shape
    R = len(res)
    want = {'sc': torch.zeros(B, L, dtype=torch.float64), 'mag': torch.zeros(B, L, dtype=torch.float64)}
    budget = {'sc': torch.zeros(B, L, dtype=torch.float64), 'mag': torch.zeros(B, L, dtype=torch.float64)}
    for n_fft, hop, win in res:
        kw = dict(n_fft=n_fft, hop=hop, win_length=win, center=True, pad_mode='reflect')
        Xr = torch.view_as_real(ST.stft_op(x.to(DEV), **kw)).cpu().numpy()
        Yr = torch.view_as_real(ST.stft_op(y.to(DEV), **kw)).cpu().numpy()
        for name, g in (('sc', (1.0, 0.0)), ('mag', (0.0, 1.0))):
            r = LH.spectral64(Xr, Yr, *g)
            G = torch.from_numpy(r['G'])
            v = LH.vjp64(G, L, n_fft, hop, win, True, 'reflect')
            yard = float((LH.adjoint_matmul(G.float(), L, n_fft, hop, win, True, 'reflect').double() - v).abs().max())
            tolG = torch.from_numpy(r['tol'][..., None] * np.abs(Xr.astype(np.float64)))
            pushed = LH.adjoint_matmul(tolG, L, n_fft, hop, win, True, 'reflect', dtype=torch.float64, absolute=True)
            want[name] += v / R
            budget[name] += (2 * yard + pushed) / R
    for name, got, from_wav in (('sc', d_sc, w_sc), ('mag', d_mag, w_mag)):
        err = (got.cpu().double() - want[name]).abs()
        top = float(want[name].abs().max())
        used = float((err / budget[name]).max())
        off = float((got.cpu().double() - from_wav).abs().max())
        print(f'{case} d {name}/dx: max-abs err {float(err.max()):.3e} of max |dx| {top:.3e}; worst sample uses {used:.3f} of its budget (<= 1; budget '
              f'{float(budget[name].min()) / top:.1e} .. {float(budget[name].max()) / top:.1e} of max |dx|); distance to the float64 gradient FROM THE '
              f'WAVEFORMS {off / float(from_wav.abs().max()):.2e} of its max (printed only)')
        assert used <= 1.0


def test_agrees_with_the_reference_modules_fixture():
    g = np.load(GOLDEN)
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    sc, mag, d_sc, d_mag = _device_run(MultiResolutionSTFTLoss(), x, y)
    for name, got, want in (('sc', float(sc), float(g['sc'])), ('mag', float(mag), float(g['mag']))):
        print(f'fixture {name}: device {got:.9f}, reference module (float32 CPU) {want:.9f}: rel {abs(got - want) / want:.2e} (bound 1e-5)')
        assert abs(got - want) <= 1e-5 * want
    for name, got, want in (('d sc/dx', d_sc, g['g_sc']), ('d mag/dx', d_mag, g['g_mag'])):
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f'fixture {name}: max-abs distance {err:.3e} = {err / float(np.abs(want).max()):.2e} of max |.| (printed only: two float32 forwards under 1 / P)')


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. determinism and capture
# ------------------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_graph_capture():
    crit = MultiResolutionSTFTLoss()
    x, y = LH.signals('near')
    x2, _ = LH.signals('silence')
    y = y.to(DEV)

    def run(wav):
        xg = wav.to(DEV).requires_grad_(True)
        sc, mag = crit(xg, y)
        dx, = torch.autograd.grad(sc + mag, xg)
        return sc.detach().clone(), mag.detach().clone(), dx.clone()

    a, b = run(x), run(x)
    assert all(torch.equal(p, q) for p, q in zip(a, b))                        # two eager calls: bitwise equal, values and dx
    eager2 = run(x2)                                                          # (also the warm-up: every basis is built)
    static = x.to(DEV).clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a host sync or a .item() inside would fail the capture itself
        sc, mag = crit(static, y)
        dx, = torch.autograd.grad(sc + mag, static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sc, a[0]) and torch.equal(mag, a[1]) and torch.equal(dx, a[2])
    with torch.no_grad():
        static.copy_(x2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sc, eager2[0]) and torch.equal(mag, eager2[1]) and torch.equal(dx, eager2[2])
    print('MultiResolutionSTFTLoss forward + backward: one captured graph, replays carry the bits of the eager calls')


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. ABI
# ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    lib = _lib.load()
    for name in ('dsv_stft_make_adjoint_basis', 'dsv_stft_adjoint_workspace_floats', 'dsv_stft_adjoint', 'dsv_spectral_loss_workspace_floats',
                 'dsv_spectral_loss', 'dsv_spectral_loss_backward'):
        assert hasattr(lib, name)
    s = torch.cuda.current_stream().cuda_stream
    adj = ST.adjoint_basis(DEV, 1024, 1024)
    assert adj.numel() == lib.dsv_stft_basis_floats(1024, 2) == 1024 * 1024
    G = torch.zeros(1, 513, 17, 2, device=DEV)
    ws = torch.zeros(lib.dsv_stft_adjoint_workspace_floats(1, 17, 1024), device=DEV)
    dx = torch.zeros(1, 4096, device=DEV)
    ok = (1, 4096, 1024, 256, 512, 512, 0)
    assert lib.dsv_stft_adjoint(G.data_ptr(), adj.data_ptr(), ws.data_ptr(), dx.data_ptr(), *ok, s) == 0
    for ptrs in ((None, adj, ws, dx), (G, None, ws, dx), (G, adj, None, dx), (G, adj, ws, None)):
        assert lib.dsv_stft_adjoint(*[p.data_ptr() if p is not None else None for p in ptrs], *ok, s) == -1
        assert b'null' in lib.dsd_last_error()
    for args, msg in (((1, 4096, 1000, 250, 500, 500, 0), b'n_fft=1000'), ((1, 4096, 1024, 0, 512, 512, 0), b'hop=0'),
                      ((1, 1023, 1024, 256, 0, 0, 0), b'shorter than one frame'), ((1, 4096, 1024, 256, 512, 512, 2), b'pad_mode'),
                      ((1, 400, 1024, 256, 512, 512, 1), b'reflect padding'), ((70000, 4096, 1024, 256, 512, 512, 0), b'B=70000'),
                      ((1, 0, 1024, 256, 512, 512, 0), b'L=0')):
        assert lib.dsv_stft_adjoint(G.data_ptr(), adj.data_ptr(), ws.data_ptr(), dx.data_ptr(), *args, s) == -1
        assert msg in lib.dsd_last_error(), (msg, lib.dsd_last_error())
    assert lib.dsv_stft_make_adjoint_basis(768, 768, adj.data_ptr(), s) == -1 and b'n_fft=768' in lib.dsd_last_error()
    assert lib.dsv_stft_make_adjoint_basis(1024, 0, adj.data_ptr(), s) == -1 and b'win_length=0' in lib.dsd_last_error()
    assert lib.dsv_stft_make_adjoint_basis(1024, 1024, None, s) == -1 and b'null' in lib.dsd_last_error()
    assert lib.dsv_stft_basis_floats(768, 2) == -1 and b'n_fft=768' in lib.dsd_last_error()
    assert lib.dsv_stft_basis_floats(1024, 3) == -1 and b'which=3' in lib.dsd_last_error()
    n = 513 * 17
    X = torch.zeros(n, 2, device=DEV)
    lw = torch.zeros(lib.dsv_spectral_loss_workspace_floats(n) // 2, device=DEV, dtype=torch.float64)
    out = torch.zeros(2, device=DEV)
    assert lib.dsv_spectral_loss(X.data_ptr(), X.data_ptr(), lw.data_ptr(), out.data_ptr(), n, s) == 0
    assert lib.dsv_spectral_loss_backward(X.data_ptr(), X.data_ptr(), lw.data_ptr(), out.data_ptr(), G.data_ptr(), n, s) == 0
    for ptrs in ((None, X, lw, out), (X, None, lw, out), (X, X, None, out), (X, X, lw, None)):
        assert lib.dsv_spectral_loss(*[p.data_ptr() if p is not None else None for p in ptrs], n, s) == -1 and b'null' in lib.dsd_last_error()
        assert lib.dsv_spectral_loss_backward(*[p.data_ptr() if p is not None else None for p in ptrs], G.data_ptr(), n, s) == -1
        assert b'null' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss_backward(X.data_ptr(), X.data_ptr(), lw.data_ptr(), out.data_ptr(), None, n, s) == -1 and b'null' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss(X.data_ptr(), X.data_ptr(), lw.data_ptr(), out.data_ptr(), 0, s) == -1 and b'n=0' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss_backward(X.data_ptr(), X.data_ptr(), lw.data_ptr(), out.data_ptr(), G.data_ptr(), -5, s) == -1 and b'n=-5' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss(X.data_ptr(), X.data_ptr(), lw.data_ptr() + 4, out.data_ptr(), n, s) == -1 and b'aligned' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss_workspace_floats(0) == -1
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0]
