"""GPU: HiFi-GAN generator training (include/dsv.h section "HiFi-GAN generator training", csrc/hifigan_train.hpp) at operator level through the C
ABI and as a whole through HifiGanGenerator.forward_train, against the restatements of tests/hifigan_train_helpers.py.

Operator tests apply the helpers' rule element-wise: |device - float64| <= 16 u sum|term|, both sides from the DEVICE'S OWN operands; where the
bound is 0 the result must be exactly 0, and [L, LS) of every written activation must be exactly 0 (outputs are pre-filled with NaN).  The
shapes are the smallest at which these kernels can go wrong: a reach beyond the signal, lengths that are no multiple of the 32-sample block,
two row blocks, one crossing of the weight gradient's split, the wide-reach instantiation.  Whole-module tests evaluate float64 on the device's
own leaky-ReLU masks and its own sine_waves.  Every float32 reference of this file runs on the CPU: no process mixes this path with torch's
eager device convolutions.  Every test prints its measured maximum beside its bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import hifigan_train_helpers as TH

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def rnd(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Ops:
    """The C ABI on torch tensors, test side (ctypes only - independent of diffsinger_amd.hifigan_train)."""

    def __init__(self):
        from diffsinger_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.split = self.lib.dsv_hgt_wgrad_split()

    def call(self, name, *args):
        self._lib.check(getattr(self.lib, name)(*args, torch.cuda.current_stream().cuda_stream), name)

    def ls(self, L):
        return self.lib.dsv_padded_samples(L)

    def padded(self, x):
        return F.pad(x.to(DEV, torch.float32), (0, self.ls(x.shape[-1]) - x.shape[-1])).contiguous()

    def pack(self, w):
        w = w.to(DEV, torch.float32).contiguous()
        rows, ci, k = w.shape
        buf = torch.empty(self.lib.dsv_packed_floats(rows, ci, k), device=DEV)
        self.call('dsv_pack_weight', w.data_ptr(), rows, ci, k, buf.data_ptr())
        return buf

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()

    def nan(self, *shape):
        return torch.full(shape, NAN, device=DEV)

    def wgrad(self, g, x, B, Co, Ci, K, pad, dil, L, up, slope):
        """dsv_hgt_conv_wgrad with a workspace of exactly the library's length -> dw [Co * up][K][Ci]"""
        n = self.lib.dsv_hgt_wgrad_workspace_floats(B, L, Co, Ci, K, up)
        ws, dw = torch.full((n,), NAN, device=DEV), self.nan(Co * up, K, Ci)
        self.call('dsv_hgt_conv_wgrad', g.data_ptr(), x.data_ptr(), ws.data_ptr(), n, dw.data_ptr(), B, Co, Ci, K, pad, dil, L, up, slope)
        return dw

    def bias(self, g, B, C, L):
        n = self.lib.dsv_hgt_bias_workspace_floats(B, C, L)
        ws, db = torch.full((n,), NAN, device=DEV), self.nan(C)
        self.call('dsv_hgt_bias_grad', g.data_ptr(), ws.data_ptr(), n, db.data_ptr(), B, C, L)
        return db


@pytest.fixture(scope='module')
def ops():
    return Ops()


def check(name, got, want, bound, L=None):
    """element-wise |got - want| <= bound on [..., :L]; exact zeros where the bound is 0 and in the padding"""
    g = TH.d64(got)
    assert bool(torch.isfinite(g).all()), f'{name}: not every element was written'
    if L is not None and g.shape[-1] > L:
        assert float(g[..., L:].abs().max()) == 0.0, f'{name}: padding columns are not zero'
        g = g[..., :L]
    err = (g - want).abs()
    k = int((err - bound).argmax())
    print(f'{name}: max err {float(err.max()):.3e}; at the tightest element err {float(err.flatten()[k]):.3e} <= bound {float(bound.flatten()[k]):.3e}')
    assert bool((err <= bound).all()), name
    zero = bound == 0
    if bool(zero.any()):
        assert float(g[zero].abs().max()) == 0.0, f'{name}: not exactly zero where every term is zero'


# ---- 1. convolution: data, weight and bias gradient ---------------------------------------------------------------------------------------------
def conv_cases():
    from diffsinger_amd import _lib
    try:
        S = _lib.load().dsv_hgt_wgrad_split()
    except Exception:                                                # collected on a machine without the library: the tests fail in the fixture
        S = 512
    return [(2, 8, 11, 5, 20), (1, 16, 7, 3, 100), (3, 32, 3, 1, S + 33), (2, 64, 11, 5, 130), (1, 128, 7, 1, 40), (1, 8, 3, 5, 1061), (1, 16, 7, 12, 90)]


@pytest.mark.parametrize('form', ['first', 'second', 'post'])
@pytest.mark.parametrize('B,C,K,dil,L', conv_cases())
def test_conv_backward(ops, B, C, K, dil, L, form):
    """first: a pair's first convolution (slope 0.1, no extras); second: with residual, sum_in and divide = 3; post: conv_post's form (C -> 1,
    slope 0.01).  (1, 16, 7, 12, 90) reaches 36 samples: the wide instantiation."""
    Co = 1 if form == 'post' else C
    slope = 0.01 if form == 'post' else 0.1
    pad = (K - 1) * dil // 2
    LS = ops.ls(L)
    seed = 1000 * C + 10 * L + K
    w = rnd(Co, C, K, seed=seed) * (C * K) ** -0.5
    g, x = ops.padded(rnd(B, Co, L, seed=seed + 1)), ops.padded(rnd(B, C, L, seed=seed + 2))
    res = ops.padded(rnd(B, C, L, seed=seed + 3)) if form == 'second' else None
    sin = ops.padded(rnd(B, C, L, seed=seed + 4)) if form == 'second' else None
    div = 3.0 if form == 'second' else 1.0
    d = lambda t: None if t is None else TH.d64(t)[..., :L]                     # noqa: E731
    dx = ops.nan(B, C, LS)
    ops.call('dsv_hgt_conv_dgrad', g.data_ptr(), ops.pack(w.flip(2).transpose(0, 1)).data_ptr(), x.data_ptr(), ops.p(res), ops.p(sin), dx.data_ptr(), B,
             Co, C, K, pad, dil, L, slope, div)
    want, bound = TH.conv_dgrad(d(g), w.double(), d(x), dil, pad, slope, d(res), d(sin), div)
    check('dx', dx, want, bound, L)
    dw = ops.wgrad(g, x, B, Co, C, K, pad, dil, L, 1, slope)
    (ww, bw), (wb, bb) = TH.conv_wgrad(d(g), d(x), K, dil, pad, slope)
    check('dw', dw.permute(0, 2, 1), ww, bw)
    check('db', ops.bias(g, B, Co, L), wb, bb)


@pytest.mark.parametrize('L', [1, 31, 513, 1061])
def test_both_weight_gradients_return_the_same_bits_where_they_state_the_same_sum(ops, L):
    """dsv_pwgt_wgrad_relu (rows 0..63 of its [128][64] block) and dsv_hgt_conv_wgrad at Co = Ci = 64, K = 1, slope 0 state the same sum
    sum_t g[co][t] relu(saved[ci][t]) on the same 512-sample splits, the same tile step and the same float64 reduction (the two kernels are
    one pattern written twice; this is the guard for folding them into one): equal bits.  (The leaky ReLU with slope 0 stages -0 where the
    ReLU stages +0; the accumulators start at +0, so no result bit sees it.)  L: one partial step, one short of a step, the split + 1, two
    splits + 37."""
    B = 2
    g, saved = ops.padded(rnd(B, 64, L, seed=7 * L + 1)), ops.padded(rnd(B, 64, L, seed=7 * L + 2))
    assert 0.3 < float((saved[..., :L] < 0).float().mean()) < 0.7
    ws = torch.full((ops.lib.dsv_pwgt_wgrad_workspace_floats(B, L, 64),), NAN, device=DEV)
    out = ops.nan(128 * 64 + 128)
    ops.call('dsv_pwgt_wgrad_relu', g.data_ptr(), saved.data_ptr(), ws.data_ptr(), out.data_ptr(), B, L)
    dw = ops.wgrad(g, saved, B, 64, 64, 1, 0, 1, L, 1, 0.0).reshape(64, 64)
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0
    assert torch.equal(out[:64 * 64].reshape(64, 64), dw)


# ---- 2. transposed convolution ------------------------------------------------------------------------------------------------------------------
def taps_of(k, u):
    """out[u q + r] takes tap j from input sample q + (r + p - j) / u, r = (j - p) mod u: per tap its phase and its column in the polyphase filter"""
    p = (k - u) // 2
    r = [(j - p) % u for j in range(k)]
    dlt = [(r[j] + p - j) // u for j in range(k)]
    return r, [v - min(dlt) for v in dlt], max(dlt) - min(dlt) + 1, -min(dlt)


def up_cases():
    S = conv_cases()[2][4] - 33
    return [(2, 128, 64, 8, 16, 9, 1.0), (1, 64, 32, 8, 16, 70, 3.0), (2, 32, 16, 2, 4, 130, 1.0), (1, 16, 8, 2, 4, S // 2 + 17, 3.0), (1, 32, 16, 4, 8, 33, 1.0)]


@pytest.mark.parametrize('B,Ci,Co,u,k,L,div', up_cases())
def test_transposed_convolution_backward(ops, B, Ci, Co, u, k, L, div):
    Lo = L * u
    seed = 7000 + 10 * L + u
    w = rnd(Ci, Co, k, seed=seed) * (Ci * k / u) ** -0.5
    g, x = ops.padded(rnd(B, Co, Lo, seed=seed + 1)), ops.padded(rnd(B, Ci, L, seed=seed + 2))
    wd = w.to(DEV).contiguous()
    dx = ops.nan(B, Ci, ops.ls(L))
    ops.call('dsv_hgt_upsample_dgrad', g.data_ptr(), wd.data_ptr(), x.data_ptr(), dx.data_ptr(), B, Ci, Co, u, k, L, 0.1, div)
    (wx, bx), (ww, bw), (wb, bb) = TH.conv_transpose_backward(TH.d64(g)[..., :Lo], TH.d64(x)[..., :L], w.double(), u, 0.1)
    check('dx', dx, wx / div, bx / div, L)
    r, t, kk, ppad = taps_of(k, u)
    dwp = ops.wgrad(g, x, B, Co, Ci, kk, ppad, 1, L, u, 0.1).view(Co, u, kk, Ci)
    check('dw', dwp[:, torch.tensor(r, device=DEV), torch.tensor(t, device=DEV), :].permute(2, 0, 1), ww, bw)
    check('db', ops.bias(g, B, Co, Lo), wb, bb)


# ---- 3. noise convolutions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Lh,stages', [(2, 640, [(64, 32, 64), (16, 2, 4)]), (1, 130, [(16, 2, 4)]), (1, 100, [(8, 1, 1)])])
def test_noise_convolution_backward(ops, B, Lh, stages):
    """dhar is accumulated over the stages in call order: the second call adds into the first's result.  Its bound is the sum of the stages'
    bounds: the one extra float32 addition rounds by u |sum| <= u sum|term|, a sixteenth of what the rule grants those terms."""
    har = ops.padded(torch.tanh(rnd(B, Lh, seed=Lh)))
    dhar = ops.nan(B, ops.ls(Lh))
    want_h, bound_h = 0.0, 0.0
    for n, (C, s, K) in enumerate(stages):
        pad = s // 2 if K > 1 else 0
        Lo = (Lh + 2 * pad - K) // s + 1
        w = rnd(C, K, seed=Lh + 10 * n + 1) * K ** -0.5
        g = ops.padded(rnd(B, C, Lo, seed=Lh + 10 * n + 2))
        dw, db = ops.nan(C, K), ops.nan(C)
        nws = ops.lib.dsv_hgt_bias_workspace_floats(B, C, Lo)
        ws = torch.full((nws,), NAN, device=DEV)
        ops.call('dsv_hgt_noise_conv_backward', g.data_ptr(), har.data_ptr(), w.to(DEV).contiguous().data_ptr(), ws.data_ptr(), nws, dw.data_ptr(), db.data_ptr(), dhar.data_ptr(),
                 B, C, K, s, pad, Lh, Lo, 1 if n == 0 else 0)
        (ww, bw), (wb, bb), (wh, bh) = TH.noise_conv_backward(TH.d64(g)[..., :Lo], TH.d64(har)[..., :Lh], w.double(), s, pad)
        check(f'dw{n}', dw, ww, bw)
        check(f'db{n}', db, wb, bb)
        want_h, bound_h = want_h + wh, bound_h + bh
        check(f'dhar after stage {n}', dhar, want_h, bound_h, Lh)


# ---- 4. source module ---------------------------------------------------------------------------------------------------------------------------
def test_source_mix_and_backward(ops):
    B, T, up, H = 2, 10, 64, 9
    L = T * up
    f0 = 180.0 + 60.0 * torch.rand(B, T, generator=torch.Generator().manual_seed(5))
    f0[0, 3:6] = 0.0                                                            # an unvoiced stretch inside
    gen = torch.Generator().manual_seed(6)
    ri, nz = torch.rand(B, H, generator=gen), torch.randn(B, L, H, generator=gen)
    lw, lb = rnd(H, seed=7) * 3.0, rnd(1, seed=8) * 0.1
    f0d, rid, nzd, lwd, lbd = (t.to(DEV).contiguous() for t in (f0, ri, nz, lw, lb))
    sw, har, sines = ops.nan(B, H, L), ops.nan(B, ops.ls(L)), ops.nan(B, L, H)
    ops.call('dsv_sine_source', f0d.data_ptr(), rid.data_ptr(), nzd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(), sw.data_ptr(), har.data_ptr(), B, T, up, H,
             24000.0, 0.1, 0.003, 0.0)
    ops.call('dsv_hgt_source_mix', f0d.data_ptr(), sw.data_ptr(), nzd.data_ptr(), sines.data_ptr(), B, T, up, H, 0.1, 0.003, 0.0)
    assert bool(torch.isfinite(sines).all())
    # the mix is k_voc_source's: uv sw + namp noise with namp = 0.003 (voiced) or 0.1 / 3 (unvoiced), two roundings
    uv = (f0 > 0).float().repeat_interleave(up, 1)[:, :, None].double()
    namp = uv * np.float32(0.003).astype(np.float64) + (1 - uv) * float(np.float32(0.1) / np.float32(3.0))
    mix = TH.d64(sw).transpose(1, 2) * uv + namp * nz.double()
    e = (TH.d64(sines) - mix).abs()
    print(f'sines: max err {float(e.max()):.3e}')
    assert bool((e <= 2 * TH.U * (mix.abs() + (namp * nz.double()).abs())).all())
    # ... and what the forward's Linear + tanh multiplied: har = tanh(sines . w + b) up to the rule on the dot product (tanh is 1-Lipschitz) + tanhf's ulps
    z = TH.d64(sines) @ lw.double() + lb.double()
    zb = TH.d64(sines).abs() @ lw.double().abs() + lb.double().abs()
    eh = (TH.d64(har)[:, :L] - torch.tanh(z)).abs()
    print(f'har: max err {float(eh.max()):.3e}, bound {float((TH.RULE * zb + 4 * TH.U).max()):.3e}')
    assert bool((eh <= TH.RULE * zb + 4 * TH.U).all()) and float(har[:, L:].abs().max() if har.shape[1] > L else 0.0) == 0.0
    dhar = ops.padded(rnd(B, L, seed=9))
    dw, db = ops.nan(H), ops.nan(1)
    ops.call('dsv_hgt_source_backward', dhar.data_ptr(), har.data_ptr(), sines.data_ptr(), dw.data_ptr(), db.data_ptr(), B, L, H)
    (ww, bw), (wb, bb) = TH.source_backward(TH.d64(dhar)[:, :L], TH.d64(har)[:, :L], TH.d64(sines))
    check('d l_linear.weight', dw, ww, bw)
    check('d l_linear.bias', db, wb, bb)


# ---- 5. conv_pre / conv_post --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 5, 33])
def test_conv_pre_and_conv_post_gradients(ops, T):
    """conv_pre at the frame rate (80 -> 32, no activation in front: slope 1); conv_post at 64 samples per frame (2 -> 1 through tanh and the
    0.01-slope leaky ReLU).  tanh backward: fl(gy fl(1 - fl(y^2))) is within 3 u |gy| of gy (1 - y^2) for |y| <= 1; 4 u |gy| is asserted."""
    B, c0 = 2, 32
    g, x = ops.padded(rnd(B, c0, T, seed=T)), ops.padded(rnd(B, 80, T, seed=T + 1))
    d = lambda t, n: TH.d64(t)[..., :n]                                         # noqa: E731
    (ww, bw), (wb, bb) = TH.conv_wgrad(d(g, T), d(x, T), 7, 1, 3, 1.0)
    check('conv_pre dw', ops.wgrad(g, x, B, c0, 80, 7, 3, 1, T, 1, 1.0).permute(0, 2, 1), ww, bw)
    check('conv_pre db', ops.bias(g, B, c0, T), wb, bb)
    L, C = 64 * T, 2
    xs = ops.padded(rnd(B, C, L, seed=T + 2))
    y = ops.padded(torch.tanh(rnd(B, 1, L, seed=T + 3)))
    gy = rnd(B, 1, L, seed=T + 4).to(DEV).contiguous()
    gp = ops.nan(B, 1, ops.ls(L))
    ops.call('dsv_hgt_tanh_backward', gy.data_ptr(), y.data_ptr(), gp.data_ptr(), B, L)
    check('tanh backward', gp, TH.d64(gy) * (1 - d(y, L) ** 2), 4 * TH.U * TH.d64(gy).abs(), L)
    w = rnd(1, C, 7, seed=T + 5) * 0.3
    (ww, bw), (wb, bb) = TH.conv_wgrad(d(gp, L), d(xs, L), 7, 1, 3, 0.01)
    check('conv_post dw', ops.wgrad(gp, xs, B, 1, C, 7, 3, 1, L, 1, 0.01).permute(0, 2, 1), ww, bw)
    check('conv_post db', ops.bias(gp, B, 1, L), wb, bb)
    dx = ops.nan(B, C, ops.ls(L))
    ops.call('dsv_hgt_conv_dgrad', gp.data_ptr(), ops.pack(w.flip(2).transpose(0, 1)).data_ptr(), xs.data_ptr(), None, None, dx.data_ptr(), B, 1, C, 7, 3, 1, L,
             0.01, 3.0)
    want, bound = TH.conv_dgrad(d(gp, L), w.double(), d(xs, L), 1, 3, 0.01, None, None, 3.0)
    check('conv_post dx', dx, want, bound, L)


# ---- 6. the whole module ------------------------------------------------------------------------------------------------------------------------
def build(h, state, removed=False):
    from diffsinger_amd.vocoder import HifiGanGenerator
    m = HifiGanGenerator(h)
    m.load_state_dict(state, strict=True)
    if removed:
        m.remove_weight_norm()
    return m.to(DEV)


def draws(seed, B, L):
    from tests.voc_helpers import draws_like_reference
    ri, nz = draws_like_reference(seed, B, L)
    return ri.to(DEV), nz.to(DEV)


def device_step(m, x, f0, dr, loss, saved=True):
    """-> (y, {key: gradient or None}, leaky-ReLU inputs, sine_waves) of one forward_train + loss + backward"""
    for p in m.parameters():
        p.grad = None
    kw = {} if dr is None else dict(rand_ini=dr[0], noise=dr[1])
    out = m.forward_train(x.to(DEV), None if f0 is None else f0.to(DEV), return_saved=saved, **kw)
    y, pre, sw = out if saved else (out, None, None)
    loss(y).backward()
    return y.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}, pre, sw


def judge(name, m, h, x, f0, dr, loss, err_of, none_keys=()):
    """One step on the device against float64 on the device's own masks and sine_waves.  err_of(state, masks, sw, grads64) -> {key: error of a
    float32 reference against grads64}."""
    y, grads, pre, sw = device_step(m, x, f0, dr, loss)
    with torch.no_grad():
        kw = {} if dr is None else dict(rand_ini=dr[0], noise=dr[1])
        assert torch.equal(m(x.to(DEV), None if f0 is None else f0.to(DEV), **kw), y), f'{name}: forward_train is not bitwise forward()'
    state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    masks = TH.masks_of(pre)
    swc = None if sw is None else sw.detach().cpu()
    o64, g64, dw64, _, _ = TH.module_grads(state, h, x, f0, loss, masks=masks, sine_waves=swc)
    assert sorted(k for k, g in grads.items() if g is None) == sorted(k for k, g in g64.items() if g is None) == sorted(none_keys)
    tol = TH.tolerances(state, g64, dw64, err_of(state, masks, swc, g64), margin=4)
    ratios = {k: float((TH.d64(grads[k]) - g64[k]).abs().max()) / tol[k] for k in tol}
    for k in sorted(ratios, key=ratios.get)[-6:]:
        print(f'{name} {k}: err / tolerance {ratios[k]:.3f} (tolerance {tol[k]:.3e}, max |grad| {float(g64[k].abs().max()):.3e})')
    bad = [k for k in ratios if ratios[k] > 1.0]
    assert not bad, bad
    return y, grads, pre, o64


def ref32_err(h, x, f0, loss):
    """err_of for judge(): the float32 restatement on the CPU on the device's masks and sine_waves against float64 on the same"""
    def err_of(state, masks, sw, g64):
        _, g32, _, _, _ = TH.module_grads(state, h, x, f0, loss, dtype=torch.float32, masks=masks, sine_waves=sw)
        return {k: float((TH.d64(g32[k]) - g64[k]).abs().max()) for k in g64 if g64[k] is not None}
    return err_of


@pytest.mark.parametrize('removed', [False, True])
@pytest.mark.parametrize('case', TH.CASES)
def test_fixture_cases(case, removed):
    """B 1, 8 frames = 512 samples.  With weight norm removed the fixture's per-tensor errors do not apply key for key: the float32 restatement
    on the device's masks is the reference error there."""
    fx = TH.fixture(case)
    h, x, f0 = fx['h'], fx['x'], fx['f0']
    loss = TH.mse_to(fx['target'])
    m = build(h, fx['state'], removed)
    dr = draws(fx['seed'], 1, x.shape[2] * TH.hop_of(h)) if f0 is not None else None
    err_of = ref32_err(h, x, f0, loss) if removed else (lambda state, masks, sw, g64: fx['err'])
    y, grads, pre, o64 = judge(f'{case}{" plain weights" if removed else ""}', m, h, x, f0, dr, loss, err_of, fx['none_keys'])
    eo = float((TH.d64(y) - TH.d64(fx['out'])).abs().max())
    lim = max(4 * fx['err_out'], TH.RULE * float(fx['out'].abs().max()))
    print(f'{case}: output against the fixture: max err {eo:.3e} <= {lim:.3e}')
    assert eo <= lim
    # mask flips against the fixture: only inputs that are tiny in the CPU float32 run, and no more than the fixture has of those
    plain = TH.plain_weights(fx['state'], h)
    torch.manual_seed(fx['seed'])
    _, pre32, _, _ = TH.generator(plain, h, x, f0, sine_waves=fx['sine_waves'])
    flips, n = TH.count_flips(TH.masks_of(pre), fx['masks'])
    small = sum(int((p.abs() < 1e-4).sum()) for p in pre32)
    print(f'{case}: {flips} of {n} masks differ from the fixture\'s; {small} inputs of the CPU float32 run are below 1e-4')
    assert n == 68352 and small == {'plain': 8, 'nsf': 5}[case] and flips <= small
    for a, b, p in zip(TH.masks_of(pre), fx['masks'], pre32):
        assert float(p[a != b].abs().max() if bool((a != b).any()) else 0.0) < 1e-4
    assert TH.count_flips(TH.masks_of(pre32), fx['masks'])[0] == 0
    if not removed:                                                  # two backward calls are bitwise equal
        y2, grads2, _, _ = device_step(m, x, f0, dr, loss)
        assert torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_resblock2():
    h = TH.config(resblock='2')
    state = TH.synth_state(TH.module_shapes(h), 51)
    x, target = rnd(2, 80, 8, seed=52), rnd(2, 1, 8 * 64, seed=53, scale=0.5)
    loss = TH.mse_to(target)
    judge('resblock2', build(h, state), h, x, None, None, loss, ref32_err(h, x, None, loss))


def test_shipped_width_nsf():
    """c0 = 128, rates [8, 8, 2, 2], kernels [16, 16, 4, 4], NSF, B 2, 5 frames = 1280 samples: the 64-row kernels and u = 8 through the module"""
    h = TH.config(use_pitch_embed=True, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=128)
    state = TH.synth_state(TH.module_shapes(h), 61)
    x, target = rnd(2, 80, 5, seed=62), rnd(2, 1, 1280, seed=63, scale=0.5)
    f0 = 200.0 + 80.0 * torch.rand(2, 5, generator=torch.Generator().manual_seed(64))
    f0[1, 1:3] = 0.0
    loss = TH.mse_to(target)
    judge('shipped width', build(h, state), h, x, f0, draws(65, 2, 1280), loss, ref32_err(h, x, f0, loss))


def test_one_capture_on_the_current_stream_replays_the_eager_bits():
    fx = TH.fixture('plain')
    m = build(fx['h'], fx['state'])
    x, target = fx['x'].to(DEV), fx['target'].to(DEV)
    params = list(m.parameters())

    def step():
        y = m.forward_train(x)
        loss = torch.mean((y - target) ** 2)
        return [y, loss] + list(torch.autograd.grad(loss, params))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # eager steps, capture and replays: all on this one stream
        eager = [t.detach().clone() for t in step()]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):                      # raises on a synchronisation or a second stream inside the region
            outs = step()
        for _ in range(2):
            for t in outs:
                t.detach().zero_()
            graph.replay()
            s.synchronize()
            assert all(torch.equal(u, v.detach()) for u, v in zip(eager, outs))
    torch.cuda.current_stream().wait_stream(s)


def test_one_step_driven_by_the_stft_loss():
    from diffsinger_amd import MultiResolutionSTFTLoss
    fx = TH.fixture('nsf')
    h = fx['h']
    m = build(h, fx['state'])
    B, T = 2, 40                                                     # 2560 samples: every shipped resolution has whole frames
    x, f0 = rnd(B, 80, T, seed=71), 220.0 + torch.zeros(B, T)
    dr = draws(72, B, T * 64)
    target = rnd(B, 1, T * 64, seed=73, scale=0.3).to(DEV)
    stft = MultiResolutionSTFTLoss().to(DEV)

    def loss(y):
        sc, mag = stft(y.squeeze(1), target.squeeze(1))
        return sc + mag
    y, grads, _, _ = device_step(m, x, f0, dr, loss, saved=False)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    leaf = y.clone().requires_grad_(True)
    cot, = torch.autograd.grad(loss(leaf), leaf)
    y2, grads2, _, _ = device_step(m, x, f0, dr, lambda out: (out * cot).sum(), saved=False)
    assert torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_refusals():
    fx = TH.fixture('plain')
    m = build(fx['h'], fx['state'])
    x = fx['x'].to(DEV)
    with pytest.raises(NotImplementedError, match='no gradient with respect to x'):
        m.forward_train(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='without use_pitch_embed'):
        m.forward_train(x, torch.zeros(1, 8, device=DEV))
    nsf = build(TH.fixture('nsf')['h'], TH.fixture('nsf')['state'])
    with pytest.raises(NotImplementedError, match='no gradient with respect to f0'):
        nsf.forward_train(x, torch.full((1, 8), 200.0, device=DEV, requires_grad=True))
