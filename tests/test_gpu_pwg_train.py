"""GPU: ParallelWaveGAN generator training (include/dsv.h section "PWG generator training", csrc/pwg_train.hpp) at operator level through the C ABI
and as a whole through ParallelWaveGANGenerator.forward_train / diffsinger_amd.pwg_train, against the restatements of tests/pwg_train_helpers.py.

Operator tests apply the helpers' rule element-wise: |device - float64| <= 16 u sum|term| (+ E_GATE terms where the gate is recomputed), both
sides from the DEVICE'S OWN operands; where the bound is 0 the result must be exactly 0, and [L, LS) of every written tensor must be exactly 0
(outputs are pre-filled with NaN).  Tiles are 32 samples and dilations reach 512: the shapes are the smallest that cross a tile boundary, leave
every outer tap outside the signal, or cross the weight gradient's split length.  Every test prints its measured maximum beside its bound."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import pwg_train_helpers as TH

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def rnd(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Ops:
    """The C ABI on torch tensors, test side (ctypes only - independent of diffsinger_amd.pwg_train)."""

    def __init__(self):
        from diffsinger_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.split = self.lib.dsv_pwgt_wgrad_split()

    def call(self, name, *args):
        self._lib.check(getattr(self.lib, name)(*args, torch.cuda.current_stream().cuda_stream), name)

    def ls(self, L):
        return self.lib.dsv_padded_samples(L)

    def padded(self, x):
        return F.pad(x.to(DEV, torch.float32), (0, self.ls(x.shape[-1]) - x.shape[-1])).contiguous()

    def pack(self, mat):
        mat = mat.to(DEV, torch.float32).contiguous()
        buf = torch.empty(self.lib.dsv_packed_floats(mat.shape[0], mat.shape[1], 1), device=DEV)
        self.call('dsv_pack_weight', mat.data_ptr(), mat.shape[0], mat.shape[1], 1, buf.data_ptr())
        return buf

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()

    def nan(self, *shape):
        return torch.full(shape, NAN, device=DEV)

    def wgrad_ws(self, B, L, n):
        return torch.empty(self.lib.dsv_pwgt_wgrad_workspace_floats(B, L, n), device=DEV)


@pytest.fixture(scope='module')
def ops():
    return Ops()


def block_weights(aux, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                 # noqa: E731
    return dict(wc=r(128, 64, 3) * (192 ** -0.5) * 2, bc=r(128) * 0.1, wa=(r(128, aux, 1) * (aux ** -0.5) if aux else None),
                wo=r(64, 64, 1) * 0.125, bo=r(64) * 0.1, ws=r(64, 64, 1) * 0.125, bs=r(64) * 0.1)


def check(name, got, want, bound, L):
    """element-wise |got - want| <= bound on [..., :L]; exact zeros where the bound is 0 and in the padding"""
    g = TH.d64(got)
    assert bool(torch.isfinite(g).all()), f'{name}: not every element was written'
    if g.shape[-1] > L:
        assert float(g[..., L:].abs().max()) == 0.0, f'{name}: padding columns are not zero'
        g = g[..., :L]
    err = (g - want).abs()
    k = int((err - bound).argmax())
    print(f'{name}: max err {float(err.max()):.3e}; at the tightest element err {float(err.flatten()[k]):.3e} <= bound {float(bound.flatten()[k]):.3e}')
    assert bool((err <= bound).all()), name
    zero = bound == 0
    if bool(zero.any()):
        assert float(g[zero].abs().max()) == 0.0, f'{name}: not exactly zero where every term is zero'


# ---- 1. training forward of a block ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,dil,aux,first', [(2, 100, 1, 80, 1), (1, 777, 4, 80, 0), (2, 1061, 512, 80, 0), (3, 65, 64, 80, 0), (1, 31, 512, 8, 1),
                                               (1, 300, 32, 0, 0)])
def test_training_forward_is_bitwise_the_inference_layer(ops, B, L, dil, aux, first):
    w = block_weights(aux, 100 + L)
    x, c = ops.padded(rnd(B, 64, L, seed=L)), (ops.padded(rnd(B, aux, L, seed=L + 1)) if aux else None)
    cols = [w['wc'].permute(0, 2, 1).reshape(128, 192)] + ([w['wa'][:, :, 0]] if aux else [])
    w1, w2 = ops.pack(torch.cat(cols, 1)), ops.pack(torch.cat([w['wo'][:, :, 0], w['ws'][:, :, 0]], 0))
    b1, b2 = w['bc'].to(DEV), torch.cat([w['bo'], w['bs']]).to(DEV)
    prev = ops.padded(rnd(B, 64, L, seed=L + 2))
    LS = ops.ls(L)
    xo, sk = ops.nan(B, 64, LS), (prev.clone() if not first else ops.nan(B, 64, LS))
    ops.call('dsv_pwg_layer', x.data_ptr(), ops.p(c), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xo.data_ptr(), sk.data_ptr(), B, L,
             aux, dil, first)
    xt, st, at = ops.nan(B, 64, LS), (prev.clone() if not first else ops.nan(B, 64, LS)), ops.nan(B, 128, LS)
    ops.call('dsv_pwgt_layer', x.data_ptr(), ops.p(c), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xt.data_ptr(), st.data_ptr(),
             at.data_ptr(), B, L, aux, dil, first)
    assert torch.equal(xo, xt) and torch.equal(sk, st)
    x64, c64 = TH.d64(x)[..., :L], (TH.d64(c)[..., :L] if aux else None)
    a = F.conv1d(x64, w['wc'].double(), w['bc'].double(), padding=dil, dilation=dil)
    ab = F.conv1d(x64.abs(), w['wc'].double().abs(), w['bc'].double().abs(), padding=dil, dilation=dil)
    if aux:
        a, ab = a + F.conv1d(c64, w['wa'].double()), ab + F.conv1d(c64.abs(), w['wa'].double().abs())
    check('a', at, a, TH.RULE * ab, L)


# ---- 2. block backward (data) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', [1, 0])
@pytest.mark.parametrize('B,L,dil,aux,last', [(2, 100, 1, 80, False), (1, 777, 4, 80, False), (2, 1500, 512, 80, False), (3, 65, 64, 80, False),
                                              (1, 31, 512, 8, False), (1, 300, 32, 0, False), (2, 100, 2, 16, True)])
def test_block_backward_data(ops, B, L, dil, aux, last, first):
    w = block_weights(aux, 200 + L)
    LS = ops.ls(L)
    dxp = None if last else ops.padded(rnd(B, 64, L, seed=L + 3))
    dS, a = ops.padded(rnd(B, 64, L, seed=L + 4)), ops.padded(rnd(B, 128, L, seed=L + 5, scale=1.5))
    assert float(a.abs().max()) <= TH.GATE_RANGE                                # the range E_GATE was computed over
    w2t = ops.pack(torch.cat([w['ws'][:, :, 0].t(), w['wo'][:, :, 0].t()], 1))
    da = ops.nan(B, 128, LS)
    ops.call('dsv_pwgt_gate_backward', ops.p(dxp), dS.data_ptr(), a.data_ptr(), w2t.data_ptr(), da.data_ptr(), B, L)
    d = lambda t: None if t is None else TH.d64(t)[..., :L]                     # noqa: E731
    want, bound = TH.gate_backward(d(dxp), d(dS), d(a), w['wo'].double(), w['ws'].double())
    check('da', da, want, bound, L)
    w1t = ops.pack(w['wc'].permute(1, 2, 0).reshape(64, 384))
    R = (aux + 31) // 32 * 32
    wat = ops.pack(F.pad(w['wa'][:, :, 0].t(), (0, 0, 0, R - aux))) if aux else None
    prev = ops.padded(rnd(B, aux, L, seed=L + 6)) if aux else None
    dc = None if not aux else (ops.nan(B, aux, LS) if first else prev.clone())
    dx = ops.nan(B, 64, LS)
    ops.call('dsv_pwgt_conv_backward', da.data_ptr(), ops.p(dxp), w1t.data_ptr(), ops.p(wat), dx.data_ptr(), ops.p(dc), B, L, aux, dil, first)
    (wx, bx), (wc_, bc_) = TH.conv_backward(d(da), d(dxp), w['wc'].double(), None if not aux else w['wa'].double(), dil,
                                            None if first or not aux else d(prev))
    check('dx', dx, wx, bx, L)
    if aux:
        check('dC', dc, wc_, bc_, L)


# ---- 3. block weight and bias gradients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dil', [1, 512])
@pytest.mark.parametrize('which', ['split-1', 'split+1', '2split+37', '7'])
def test_block_weight_gradients(ops, which, dil):
    L = {'7': 7, 'split-1': ops.split - 1, 'split+1': ops.split + 1, '2split+37': 2 * ops.split + 37}[which]
    B, aux = 2, 16
    n1 = 192 + aux
    da, x, c = ops.padded(rnd(B, 128, L, seed=L + 7)), ops.padded(rnd(B, 64, L, seed=L + 8)), ops.padded(rnd(B, aux, L, seed=L + 9))
    ws = ops.wgrad_ws(B, L, n1)
    out = ops.nan(128 * n1 + 128)
    ops.call('dsv_pwgt_wgrad_conv', da.data_ptr(), x.data_ptr(), c.data_ptr(), ws.data_ptr(), out.data_ptr(), B, L, aux, dil)
    d = lambda t: TH.d64(t)[..., :L]                                            # noqa: E731
    (dw, bw), (db, bb) = TH.wgrad_conv(d(da), d(x), d(c), dil)
    check('dW1', out[:128 * n1].reshape(128, n1), dw, bw, n1)
    check('db1', out[128 * n1:], db, bb, 128)
    if dil >= L:                                                               # the outer taps never meet the signal: exact zeros
        got = out[:128 * n1].reshape(128, n1)
        assert float(got[:, :64].abs().max()) == 0.0 and float(got[:, 128:192].abs().max()) == 0.0 and float(got[:, 64:128].abs().max()) > 0
    dxp, dS, a = ops.padded(rnd(B, 64, L, seed=L + 10)), ops.padded(rnd(B, 64, L, seed=L + 11)), ops.padded(rnd(B, 128, L, seed=L + 12, scale=1.5))
    assert float(a.abs().max()) <= TH.GATE_RANGE
    for name, dx_ in (('dW2', dxp), ('dW2 (last block)', None)):
        out2 = ops.nan(128 * 64 + 128)
        ops.call('dsv_pwgt_wgrad_out', ops.p(dx_), dS.data_ptr(), a.data_ptr(), ws.data_ptr(), out2.data_ptr(), B, L)
        (dw, bw), (db, bb) = TH.wgrad_out(None if dx_ is None else d(dx_), d(dS), d(a))
        check(name, out2[:128 * 64].reshape(128, 64), dw, bw, 64)
        check(name + ' bias', out2[128 * 64:], db, bb, 128)
    g, saved = ops.padded(rnd(B, 64, L, seed=L + 13)), ops.padded(rnd(B, 64, L, seed=L + 14))
    out3 = ops.nan(128 * 64 + 128)
    ops.call('dsv_pwgt_wgrad_relu', g.data_ptr(), saved.data_ptr(), ws.data_ptr(), out3.data_ptr(), B, L)
    (dw, bw), (db, bb) = TH.wgrad_relu(d(g), d(saved))
    check('dW last1', out3[:64 * 64].reshape(64, 64), dw, bw, 64)
    check('db last1', out3[128 * 64:128 * 64 + 64], db, bb, 64)
    assert float(out3[64 * 64:128 * 64].abs().max()) == 0.0 and float(out3[128 * 64 + 64:].abs().max()) == 0.0


# ---- 4. upsampling network ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,scale', [(1, 4), (7, 4), (33, 2), (100, 8)])
def test_upsample_stage_backward(ops, L, scale):
    B, aux = 2, 8
    g, inp, filt = ops.padded(rnd(B, aux, L * scale, seed=L + 15)), ops.padded(rnd(B, aux, L, seed=L + 16)), rnd(2 * scale + 1, seed=L + 17).to(DEV)
    ws = torch.empty(ops.lib.dsv_pwgt_upsample_workspace_floats(B * aux, scale) // 2, device=DEV, dtype=torch.float64)
    din, dw = ops.nan(B, aux, ops.ls(L)), ops.nan(2 * scale + 1)
    ops.call('dsv_pwgt_upsample_backward', g.data_ptr(), inp.data_ptr(), filt.data_ptr(), ws.data_ptr(), din.data_ptr(), dw.data_ptr(), B * aux, L, scale)
    (wi, bi), (wf, bf) = TH.upsample_backward(TH.d64(g)[..., :L * scale], TH.d64(inp)[..., :L], TH.d64(filt), scale)
    check('din', din, wi, bi, L)
    check('dfilter', dw, wf, bf, 2 * scale + 1)
    dw2 = ops.nan(2 * scale + 1)                                               # without the data gradient: one launch less, the same filter gradient
    ops.call('dsv_pwgt_upsample_backward', g.data_ptr(), inp.data_ptr(), filt.data_ptr(), ws.data_ptr(), None, dw2.data_ptr(), B * aux, L, scale)
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize('frames', [1, 7])
def test_conv_in_weight_gradient(ops, frames):
    B, aux, K = 2, 16, 5
    g, c = ops.padded(rnd(B, aux, frames, seed=frames + 18)), ops.padded(rnd(B, aux, frames + K - 1, seed=frames + 19))
    dw = ops.nan(aux, aux, K)
    ops.call('dsv_pwgt_convin_wgrad', g.data_ptr(), c.data_ptr(), dw.data_ptr(), B, aux, K, frames)
    want, bound = TH.convin_wgrad(TH.d64(g)[..., :frames], TH.d64(c)[..., :frames + K - 1])
    check('d conv_in', dw, want, bound, K)


# ---- 5. first_conv and last_conv_layers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 33])
def test_first_and_last_layer_gradients(ops, T):
    B = 2
    LS = ops.ls(T)
    d = lambda t: TH.d64(t)[..., :T]                                            # noqa: E731
    # first_conv: dw0[c] = sum dx0[c][t] z[t], db0[c] = sum dx0[c][t]
    dx0, z = ops.padded(rnd(B, 64, T, seed=T + 20)), ops.padded(rnd(B, 1, T, seed=T + 21))
    out = ops.nan(128)
    ops.call('dsv_pwgt_rowdot', dx0.data_ptr(), z.data_ptr(), out.data_ptr(), B, 64, T, 1, 0, 0)
    check('d first_conv.weight', out[0::2], (d(dx0) * d(z)).sum((0, 2)), TH.RULE * (d(dx0) * d(z)).abs().sum((0, 2)), 64)
    check('d first_conv.bias', out[1::2], d(dx0).sum((0, 2)), TH.RULE * d(dx0).abs().sum((0, 2)), 64)
    # last_conv_layers[3] (64 -> 1) behind its ReLU
    gy, o1, w3 = ops.padded(rnd(B, 1, T, seed=T + 22)), ops.padded(rnd(B, 64, T, seed=T + 23)), rnd(64, seed=T + 24).to(DEV)
    out = ops.nan(128)
    ops.call('dsv_pwgt_rowdot', gy.data_ptr(), o1.data_ptr(), out.data_ptr(), B, 64, T, 0, 1, 1)
    r = torch.relu(d(o1))
    check('d last3.weight', out[0::2], (d(gy) * r).sum((0, 2)), TH.RULE * (d(gy) * r).abs().sum((0, 2)), 64)
    check('d last3.bias', out[1:2], d(gy).sum().reshape(1), TH.RULE * d(gy).abs().sum().reshape(1), 1)
    do1 = ops.nan(B, 64, LS)
    ops.call('dsv_pwgt_last_dgrad', gy.data_ptr(), o1.data_ptr(), w3.data_ptr(), do1.data_ptr(), B, 64, T)
    want = TH.d64(w3)[None, :, None] * d(gy) * (d(o1) > 0)
    check('d o1', do1, want, 2 * TH.U * want.abs(), T)
    # the ReLU in front of last_conv_layers[1] and the skip sum's scale
    g, saved, scale = ops.padded(rnd(B, 64, T, seed=T + 25)), ops.padded(rnd(B, 64, T, seed=T + 26)), math.sqrt(1.0 / 30)
    dS = ops.nan(B, 64, LS)
    ops.call('dsv_pwgt_relu_mask', g.data_ptr(), saved.data_ptr(), dS.data_ptr(), scale, B * 64, T)
    want = d(g) * (d(saved) > 0) * scale
    check('dS', dS, want, 2 * TH.U * want.abs(), T)


# ---- 6. the whole module ---------------------------------------------------------------------------------------------------------------------------
def build(cfg, state, plain=False):
    from diffsinger_amd.pwg import ParallelWaveGANGenerator
    m = ParallelWaveGANGenerator(layers=cfg['layers'], stacks=cfg['stacks'], aux_channels=cfg['aux'], aux_context_window=cfg['ctx'],
                                 upsample_params={'upsample_scales': list(cfg['scales'])}, bias=cfg['bias'])
    m.load_state_dict(state, strict=True)
    m = m.to(DEV)
    if plain:
        m.remove_weight_norm()                                                 # on the device: the same g v / |v| kernel the weight-normed form runs
    return m


def device_grads(m, x, c, loss_of):
    for p in m.parameters():
        p.grad = None
    y = m.forward_train(x.to(DEV), c.to(DEV))
    loss_of(y).backward()
    return y.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def torch32(state, x, c, cfg, loss):
    """the restatement in float32 through torch on the device (its native convolution kernels: no library search for the dilated shapes)"""
    with torch.backends.cudnn.flags(enabled=False):
        return TH.module_grads(state, x, c, cfg, loss, dtype=torch.float32, device=DEV)


@pytest.fixture(scope='module')
def fx():
    f = TH.fixture()
    f['ref64'] = TH.module_grads(f['state'], f['x'], f['c'], f['cfg'], TH.mse_to(f['target']))
    return f


def test_whole_module_against_the_reference_fixture(fx):
    m = build(fx['cfg'], fx['state'])
    y, grads = device_grads(m, fx['x'], fx['c'], TH.mse_to(fx['target']))
    assert y.dtype == torch.float32 and tuple(y.shape) == tuple(fx['out'].shape)
    err = float((y.cpu() - fx['out']).abs().max())
    print(f'output: max err {err:.3e} against the reference (tolerance 2e-5)')
    assert err <= 2e-5
    assert sorted(k for k, g in grads.items() if g is None) == sorted(fx['none_keys'])
    _, g64, dw64 = fx['ref64']
    tol = TH.tolerances(fx['state'], g64, dw64, fx['err'])
    worst = 0.0
    for k in sorted(tol):
        e = float((TH.d64(grads[k]) - fx['grads'][k].double()).abs().max())
        worst = max(worst, e / tol[k])
        print(f'{k}: max err {e:.3e} <= {tol[k]:.3e} (ratio {e / tol[k]:.2f}; 4 x err_ref32 = {4 * fx["err"][k]:.3e})')
        assert e <= tol[k], k
    print(f'worst ratio {worst:.2f}')
    with torch.no_grad():
        assert torch.equal(m(fx['x'].to(DEV), fx['c'].to(DEV)), y)            # forward_train is bitwise forward()


def test_plain_form_agrees_with_the_weight_normed_form(fx):
    """after remove_weight_norm() the gradients of the plain weights, sent through the weight-norm expression in float64, are the weight-normed
    module's gradients within the rule of that expression; biases are bitwise equal (the same kernels on the same plain weights)."""
    loss = TH.mse_to(fx['target'])
    y1, g1 = device_grads(build(fx['cfg'], fx['state']), fx['x'], fx['c'], loss)
    y2, g2 = device_grads(build(fx['cfg'], fx['state'], plain=True), fx['x'], fx['c'], loss)
    assert torch.equal(y1, y2)
    for p, _, hb in TH.module_prefixes(fx['cfg']):
        if g2[p + 'weight'] is None:
            assert g1[p + 'weight_g'] is None and g1[p + 'weight_v'] is None and g1.get(p + 'bias') is None and g2.get(p + 'bias') is None
            continue
        if hb:
            assert torch.equal(g1[p + 'bias'], g2[p + 'bias']), p
        g, v = TH.d64(fx['state'][p + 'weight_g']).requires_grad_(True), TH.d64(fx['state'][p + 'weight_v']).requires_grad_(True)
        dw = TH.d64(g2[p + 'weight'])
        TH.weight_norm(g, v).backward(dw)
        bg, bv = TH.weight_norm_bounds(g.detach(), v.detach(), dw)
        for name, got, want, bound in ((p + 'weight_g', g1[p + 'weight_g'], g.grad, bg), (p + 'weight_v', g1[p + 'weight_v'], v.grad, bv)):
            e = (TH.d64(got) - want).abs()
            print(f'{name}: max err {float(e.max()):.3e}, max bound {float(bound.max()):.3e}')
            assert bool((e <= bound).all()), name


@pytest.mark.parametrize('B,frames', [(1, 5), (3, 7)])
def test_shipped_thirty_layers_against_float64(B, frames):
    """layers 30 / stacks 3 / aux 80.  B = 1, 5 frames (T = 1280: dilation 512 is live, one weight-gradient split), and B = 3, 7 frames
    (T = 1792: three batch rows of three whole splits and a partial one - the partials of 12 workgroups per column group are reduced).  Against
    the helper's float64 on the device's own parameters; per tensor 4 x the error of the SAME restatement run in float32 through torch on the
    device, floor 16 u max|grad64|."""
    cfg = TH.config()
    state = TH.synth_state(TH.module_shapes(cfg), 31)
    m = build(cfg, state)
    T = 256 * frames
    x, c, target = rnd(B, 1, T, seed=32), rnd(B, 80, frames + 4, seed=33), rnd(B, 1, T, seed=34, scale=0.5)
    loss = TH.mse_to(target)
    y, grads = device_grads(m, x, c, loss)
    dstate = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    o64, g64, dw64 = TH.module_grads(dstate, x, c, cfg, loss)
    o32, g32, _ = torch32(dstate, x, c, cfg, loss)
    eo = float((TH.d64(o32) - o64).abs().max())
    e = float((TH.d64(y) - o64).abs().max())
    print(f'output: max err {e:.3e}; torch float32 on the device {eo:.3e} (max |y| {float(o64.abs().max()):.3f})')
    assert e <= max(4 * eo, TH.RULE * float(o64.abs().max()))
    assert sorted(k for k, g in grads.items() if g is None) == sorted(k for k, g in g64.items() if g is None) == [
        'conv_layers.29.conv1x1_out.bias', 'conv_layers.29.conv1x1_out.weight_g', 'conv_layers.29.conv1x1_out.weight_v']
    err32 = {k: float((TH.d64(g32[k]) - g64[k]).abs().max()) for k in g64 if g64[k] is not None}
    tol = TH.tolerances(dstate, g64, dw64, err32)
    ratios = {k: float((TH.d64(grads[k]) - g64[k]).abs().max()) / tol[k] for k in tol}
    worst = sorted(ratios, key=ratios.get)[-8:]
    for k in worst:
        print(f'{k}: err / tolerance {ratios[k]:.2f} (torch float32 err {err32[k]:.3e}, max |grad| {float(g64[k].abs().max()):.3e})')
    bad = [k for k in ratios if ratios[k] > 1.0]
    assert not bad, bad
    with torch.no_grad():
        assert torch.equal(m(x.to(DEV), c.to(DEV)), y)


def test_bias_off_and_two_steps_bitwise():
    cfg = TH.config(layers=4, stacks=2, aux=8, scales=(4, 4), bias=False)
    state = TH.synth_state(TH.module_shapes(cfg), 35)
    m = build(cfg, state)
    x, c, target = rnd(2, 1, 16 * 7, seed=36), rnd(2, 8, 11, seed=37), rnd(2, 1, 16 * 7, seed=38)
    loss = TH.mse_to(target)
    y1, g1 = device_grads(m, x, c, loss)
    y2, g2 = device_grads(m, x, c, loss)
    assert torch.equal(y1, y2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k
    o64, g64, dw64 = TH.module_grads(state, x, c, cfg, loss)
    _, g32, _ = torch32(state, x, c, cfg, loss)
    err32 = {k: float((TH.d64(g32[k]) - g64[k]).abs().max()) for k in g64 if g64[k] is not None}
    tol = TH.tolerances(state, g64, dw64, err32)
    assert {k for k in g1 if g1[k] is not None} == set(tol)
    for k in tol:
        e = float((TH.d64(g1[k]) - g64[k]).abs().max())
        assert e <= tol[k], (k, e, tol[k])
    with torch.no_grad():
        assert torch.equal(m(x.to(DEV), c.to(DEV)), y1)
    # return_saved: the same waveform, and the inputs of the two ReLUs of last_conv_layers (the backward takes their masks from these)
    y3, (S, o1) = m.forward_train(x.to(DEV), c.to(DEV), return_saved=True)
    assert torch.equal(y3, y1) and tuple(S.shape) == tuple(o1.shape) == (2, 64, 16 * 7) and not S.requires_grad and not o1.requires_grad
    plain = {p + 'weight': TH.d64(state[p + 'weight_g']) * TH.d64(state[p + 'weight_v']) / TH.d64(state[p + 'weight_v']).flatten(1).norm(dim=1).reshape(
        state[p + 'weight_g'].shape) for p, _, _ in TH.module_prefixes(cfg)}
    plain['last_conv_layers.1.bias'] = TH.d64(state['last_conv_layers.1.bias'])
    want = F.conv1d(torch.relu(TH.d64(S)), plain['last_conv_layers.1.weight'], plain['last_conv_layers.1.bias'])
    assert float((TH.d64(o1) - want).abs().max()) <= TH.RULE * float(F.conv1d(torch.relu(TH.d64(S)), plain['last_conv_layers.1.weight'].abs(),
                                                                           plain['last_conv_layers.1.bias'].abs()).max())


# ---- 7. the objectives -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trainer(fx):
    from diffsinger_amd import MultiResolutionSTFTLoss, ParallelWaveGANDiscriminator
    from tests import pwg_disc_helpers as DH
    gen = build(fx['cfg'], fx['state'])
    disc = ParallelWaveGANDiscriminator(layers=10)
    disc.load_state_dict(DH.synth_state(DH.module_shapes(10), 41), strict=True)
    stft = MultiResolutionSTFTLoss()                                           # the shipped resolutions (configs/tts/pwg.yaml stft_loss_params)
    B, T = 2, 2560
    batch = dict(x=rnd(B, 1, T, seed=42).to(DEV), c=rnd(B, 16, T // 256 + 4, seed=43).to(DEV), y=rnd(B, 1, T, seed=44, scale=0.3).to(DEV))
    return gen, disc.to(DEV), stft.to(DEV), batch


def _zero(*mods):
    for m in mods:
        for p in m.parameters():
            p.grad = None


def test_objectives_are_the_composition_of_the_public_operators(trainer):
    from diffsinger_amd import discriminator_loss, generator_loss, pwg_discriminator_losses, pwg_generator_losses
    gen, disc, stft, b = trainer
    _zero(gen, disc)
    losses, y_ = pwg_generator_losses(gen, disc, stft, b['x'], b['c'], b['y'], lambda_adv=4.0, adversarial=True)
    losses['total'].backward()
    got = [p.grad.clone() for p in gen.parameters() if p.grad is not None]
    assert any(p.grad is not None for p in disc.parameters())
    _zero(gen, disc)
    y2 = gen.forward_train(b['x'], b['c'])
    sc, mag = stft(y2.squeeze(1), b['y'].squeeze(1))
    adv = generator_loss([disc(y2)])
    total = sc + mag + 4.0 * adv
    total.backward()
    want = [p.grad.clone() for p in gen.parameters() if p.grad is not None]
    assert torch.equal(y_, y2) and torch.equal(losses['sc'], sc) and torch.equal(losses['mag'], mag) and torch.equal(losses['adv'], adv)
    assert torch.equal(losses['total'], total)
    assert len(got) == len(want) and all(torch.equal(u, v) for u, v in zip(got, want))
    # without the adversarial term the discriminator is not touched
    _zero(gen, disc)
    l2, _ = pwg_generator_losses(gen, disc, stft, b['x'], b['c'], b['y'], lambda_adv=4.0, adversarial=False)
    assert 'adv' not in l2 and torch.equal(l2['total'], sc + mag)
    l2['total'].backward()
    assert all(p.grad is None for p in disc.parameters())
    # the discriminator's objective: on the detached waveform
    _zero(gen, disc)
    dl = pwg_discriminator_losses(disc, b['y'], y_)
    dl['total'].backward()
    assert all(p.grad is None for p in gen.parameters()) and all(p.grad is not None for p in disc.parameters())
    real, fake = discriminator_loss([disc(b['y'])], [disc(y_.detach())])
    assert torch.equal(dl['real'], real) and torch.equal(dl['fake'], fake) and torch.equal(dl['total'], real + fake)


def _norm(params):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)))


def test_training_step_schedule_and_clipping(trainer):
    from diffsinger_amd import pwg_training_step
    gen, disc, stft, b = trainer
    hp = dict(lambda_adv=4.0, generator_grad_norm=1e-3, discriminator_grad_norm=1e-4, disc_start_steps=5)
    g0 = [p.detach().clone() for p in gen.parameters()]
    d0 = [p.detach().clone() for p in disc.parameters()]
    opt_g, opt_d = torch.optim.SGD(gen.parameters(), lr=1.0), torch.optim.SGD(disc.parameters(), lr=1.0)
    try:
        out = pwg_training_step(gen, disc, stft, b, hp, 4, opt_g, opt_d)      # before disc_start_steps: no adversarial term, no discriminator step
        assert 'gen_adv' not in out and 'disc_total' not in out
        assert all(p.grad is None for p in disc.parameters()) and all(torch.equal(u, v) for u, v in zip(d0, disc.parameters()))
        assert float(out['gen_grad_norm']) > hp['generator_grad_norm']
        assert abs(_norm(gen.parameters()) / hp['generator_grad_norm'] - 1.0) < 1e-3          # clipped to the configured norm
        assert any(not torch.equal(u, v) for u, v in zip(g0, gen.parameters()))               # the generator stepped
        out = pwg_training_step(gen, disc, stft, b, hp, 5, opt_g, opt_d)      # from disc_start_steps on: both
        assert 'gen_adv' in out and 'disc_total' in out and torch.equal(out['disc_total'], out['disc_real'] + out['disc_fake'])
        assert float(out['disc_grad_norm']) > hp['discriminator_grad_norm']
        assert abs(_norm(disc.parameters()) / hp['discriminator_grad_norm'] - 1.0) < 1e-3
        assert any(not torch.equal(u, v) for u, v in zip(d0, disc.parameters()))
        out2 = pwg_training_step(gen, disc, stft, b, dict(hp, generator_grad_norm=1e9, discriminator_grad_norm=1e9), 5)      # no optimisers, no clipping
        assert abs(_norm(gen.parameters()) / float(out2['gen_grad_norm']) - 1.0) < 1e-5
    finally:
        with torch.no_grad():
            for p, v in zip(list(gen.parameters()) + list(disc.parameters()), g0 + d0):
                p.copy_(v)
        _zero(gen, disc)


def test_one_graph_capture_replays_the_eager_bits(trainer):
    from diffsinger_amd import pwg_generator_losses
    gen, disc, stft, b = trainer
    params = [p for k, p in gen.named_parameters() if 'conv_layers.3.conv1x1_out' not in k]

    def step():
        losses, y_ = pwg_generator_losses(gen, disc, stft, b['x'], b['c'], b['y'], lambda_adv=4.0, adversarial=True)
        return [y_, losses['total'], losses['sc'], losses['mag'], losses['adv']] + list(torch.autograd.grad(losses['total'], params))

    a = [t.detach().clone() for t in step()]
    again = [t.detach().clone() for t in step()]
    assert all(torch.equal(u, v) for u, v in zip(a, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                 # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                              # raises on a synchronisation inside the region
        outs = step()
    for _ in range(2):
        for t in outs:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v.detach()) for u, v in zip(a, outs))
