"""Test infrastructure of ParallelWaveGAN generator training (include/dsv.h, section "PWG generator training"): restatements on explicit tensors,
written from the reference's lines (modules/parallel_wavegan/models/parallel_wavegan.py:139-177, layers/residual_block.py:96-129,
layers/upsample.py:96-183) and independent of the product code, and the error rule the tests apply to them.

THE RULE (tests/pwg_disc_helpers.py).  u = 2^-24.  A result that is an fp32 sum of products may differ from float64 by at most
RULE sum|term| = 16 u sum|term| element-wise, sum|term| being the same sum over absolute values in float64.  Every operator function below
returns (value, bound) pairs built this way from the operands it is given (the device's own operands in the GPU tests: exact inputs).

THE GATE.  The kernels evaluate tanh(a) = 1 - 2 / (e^(2a) + 1) and sigmoid(g) = 1 / (1 + e^-g) in float32 on the hardware exponential, and
the backward recomputes them, z = tanh sigmoid and the two derivative factors sigmoid (1 - tanh^2) and tanh sigmoid (1 - sigmoid) from the
saved pre-activations.  These carry an ABSOLUTE error that u sum|term| does not cover (1 - tanh^2 cancels).  E_GATE is computed here, not
guessed: the largest error, over a grid of a, g in [-12, 12] and over seeded random points, of exactly those float32 formulas evaluated
with numpy float32 (libm's exponential, every operation rounded to float32 in the kernel's order) against the same formulas in float64 -
DOUBLED, because the device exponential rounds differently from libm.  A gate-gradient element may be off by E_GATE |dz| more than the
rule, a weight gradient against the recomputed z by E_GATE sum|G| more."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
RULE = 16.0 * U
S = math.sqrt(0.5)
RES, GATE = 64, 128
GATE_RANGE = 12.0                         # |a|, |g| over which E_GATE is computed; a test that applies E_GATE asserts its pre-activations lie inside


def _gate_error_constant():
    f32 = np.float32
    grid = np.linspace(-GATE_RANGE, GATE_RANGE, 1601).astype(f32)
    rng = np.random.RandomState(20240611)
    a = np.concatenate([np.repeat(grid, grid.size), rng.uniform(-GATE_RANGE, GATE_RANGE, 400000).astype(f32)])
    g = np.concatenate([np.tile(grid, grid.size), rng.uniform(-GATE_RANGE, GATE_RANGE, 400000).astype(f32)])
    one, two = f32(1.0), f32(2.0)
    th = one - two / (np.exp(two * a) + one)
    sg = one / (one + np.exp(-g))
    z, f1, f2 = th * sg, sg * (one - th * th), th * (sg * (one - sg))
    assert th.dtype == f32 and f1.dtype == f32 and f2.dtype == f32
    a64, g64 = a.astype(np.float64), g.astype(np.float64)
    th64, sg64 = np.tanh(a64), 1.0 / (1.0 + np.exp(-g64))
    err = max(np.abs(th - th64).max(), np.abs(sg - sg64).max(), np.abs(z - th64 * sg64).max(), np.abs(f1 - sg64 * (1.0 - th64 * th64)).max(),
              np.abs(f2 - th64 * sg64 * (1.0 - sg64)).max())
    return 2.0 * float(err)


E_GATE = _gate_error_constant()            # about 7.4e-7: a few float32 roundings of values of magnitude <= 1 (the largest: tanh), doubled


def d64(t):
    return t.detach().to('cpu', torch.float64)


def weight_norm(g, v):
    return g * v / v.flatten(1).norm(dim=1).reshape(g.shape)


# ---- the module on explicit tensors (any dtype / device; differentiable) ---------------------------------------------------------------------
def config(layers=30, stacks=3, aux=80, scales=(4, 4, 4, 4), ctx=2, bias=True):
    return dict(layers=layers, stacks=stacks, aux=aux, scales=list(scales), ctx=ctx, bias=bias)


def dilation_of(i, cfg):
    return 2 ** (i % (cfg['layers'] // cfg['stacks']))


def module_prefixes(cfg):
    """parameter holders in the module's own order: (prefix, weight shape, has bias)"""
    aux, b = cfg['aux'], cfg['bias']
    out = [('first_conv.', (RES, 1, 1), True), ('upsample_net.conv_in.', (aux, aux, 2 * cfg['ctx'] + 1), False)]
    out += [(f'upsample_net.upsample.up_layers.{2 * i + 1}.', (1, 1, 1, 2 * s + 1), False) for i, s in enumerate(cfg['scales'])]
    for i in range(cfg['layers']):
        p = f'conv_layers.{i}.'
        out += [(p + 'conv.', (GATE, RES, 3), b), (p + 'conv1x1_aux.', (GATE, aux, 1), False), (p + 'conv1x1_out.', (RES, RES, 1), b),
                (p + 'conv1x1_skip.', (RES, RES, 1), b)]
    return out + [('last_conv_layers.1.', (RES, RES, 1), True), ('last_conv_layers.3.', (1, RES, 1), True)]


def module_shapes(cfg, weight_norm_on=True):
    out = {}
    for p, shp, hb in module_prefixes(cfg):
        if hb:
            out[p + 'bias'] = (shp[0],)
        if weight_norm_on:
            out[p + 'weight_g'] = (shp[0],) + (1,) * (len(shp) - 1)
            out[p + 'weight_v'] = shp
        else:
            out[p + 'weight'] = shp
    return out


def synth_state(shapes, seed):
    """(The fixture holds this state ROUNDED TO FLOAT16 - `v.half().float()`, tools/make_golden_pwg_train.py - so synth_state(shapes, seed) alone does
    not reproduce it.)  A seeded O(1) state (the module's 0.01-scale initialisation makes every gradient vanish): weight_v ~ N(0, 1 / fan_in), weight_g uniform
    in [0.7, 1.3], biases 0.1 N(0, 1); a plain weight has rows of norm in [0.7, 1.3]."""
    gen = torch.Generator().manual_seed(seed)
    st = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith('bias'):
            st[k] = 0.1 * torch.randn(shp, generator=gen)
        elif k.endswith('weight_g'):
            st[k] = 0.7 + 0.6 * torch.rand(shp, generator=gen)
        elif k.endswith('weight_v'):
            st[k] = torch.randn(shp, generator=gen) / math.sqrt(float(np.prod(shp[1:])))
        else:
            w = torch.randn(shp, generator=gen)
            gsh = (shp[0],) + (1,) * (len(shp) - 1)
            st[k] = (0.7 + 0.6 * torch.rand(gsh, generator=gen)) * w / w.flatten(1).norm(dim=1).reshape(gsh)
    return st


def upsample(c, filt, scale):
    """one stage of UpsampleNetwork: nearest-neighbour stretch + the (1, 2 scale + 1) smoothing filter, zero padded"""
    B, A, L = c.shape
    y = c.repeat_interleave(scale, dim=2).reshape(B * A, 1, L * scale)
    return F.conv1d(y, filt.reshape(1, 1, -1), padding=scale).reshape(B, A, L * scale)


def block(h, cond, wc, bc, wa, wo, bo, wsk, bsk, dil):
    """ResidualBlock.forward -> (a, z, x', skip)"""
    a = F.conv1d(h, wc, bc, padding=dil, dilation=dil)
    if wa is not None:
        a = a + F.conv1d(cond, wa)
    z = torch.tanh(a[:, :RES]) * torch.sigmoid(a[:, RES:])
    return a, z, (F.conv1d(z, wo, bo) + h) * S, F.conv1d(z, wsk, bsk)


def generator(plain, x, c, cfg):
    """ParallelWaveGANGenerator.forward on a dict of plain weights {prefix + 'weight' / 'bias'}"""
    def wb(p):
        return plain[p + 'weight'], plain.get(p + 'bias')
    y = F.conv1d(c, plain['upsample_net.conv_in.weight'])
    for i, s in enumerate(cfg['scales']):
        y = upsample(y, plain[f'upsample_net.upsample.up_layers.{2 * i + 1}.weight'], s)
    h = F.conv1d(x, *wb('first_conv.'))
    skips = 0
    for i in range(cfg['layers']):
        p = f'conv_layers.{i}.'
        _, _, h, sk = block(h, y, *wb(p + 'conv.'), plain[p + 'conv1x1_aux.weight'], *wb(p + 'conv1x1_out.'), *wb(p + 'conv1x1_skip.'),
                            dilation_of(i, cfg))
        skips = skips + sk
    skips = skips * math.sqrt(1.0 / cfg['layers'])
    o = F.conv1d(torch.relu(skips), *wb('last_conv_layers.1.'))
    return F.conv1d(torch.relu(o), *wb('last_conv_layers.3.'))


def module_grads(state, x, c, cfg, loss_of, dtype=torch.float64, device='cpu'):
    """The module's output and the gradient of loss_of(output) with respect to every tensor of `state` (weight-normed or plain form), by autograd
    over the restatement in `dtype` on `device`.  -> (out, grads {key: tensor or None}, dw {prefix: gradient of the plain weight or None})"""
    leaves = {k: v.detach().to(device, dtype).clone().requires_grad_(True) for k, v in state.items()}
    plain = {}
    for p, _, hb in module_prefixes(cfg):
        if p + 'weight' in leaves:
            plain[p + 'weight'] = leaves[p + 'weight']
        else:
            w = weight_norm(leaves[p + 'weight_g'], leaves[p + 'weight_v'])
            w.retain_grad()
            plain[p + 'weight'] = w
        if hb:
            plain[p + 'bias'] = leaves[p + 'bias']
    out = generator(plain, x.detach().to(device, dtype), c.detach().to(device, dtype), cfg)
    loss_of(out).backward()
    grads = {k: (None if v.grad is None else v.grad.detach()) for k, v in leaves.items()}
    dw = {p: (None if plain[p + 'weight'].grad is None else plain[p + 'weight'].grad.detach()) for p, _, _ in module_prefixes(cfg)}
    return out.detach(), grads, dw


def weight_norm_bounds(g, v, dw):
    """RULE times the sums of absolute terms of the gradients of w = g v / ||v|| given dL/dw (float64) -> (bound of dg, bound of dv): what the
    float32 weight-norm expression may add to the error of a weight_g / weight_v gradient whatever the tensor's own magnitude (the gradient of
    a one-element row's weight_v is mathematically zero)."""
    nrm = v.flatten(1).norm(dim=1).reshape(g.shape)
    va, ga, d = v.abs(), g.abs(), dw.abs()
    s = (d * va).flatten(1).sum(1).reshape(g.shape)
    return RULE * s / nrm, RULE * (ga / nrm * d + ga * s / nrm ** 3 * va)


def tolerances(state, grads64, dw64, err_ref32, margin=4.0):
    """per-tensor tolerance of a float32 gradient against grads64: margin * err_ref32 with the floor RULE max|grad64|, plus for weight_g / weight_v
    the rule of the weight-norm expression itself"""
    tol = {}
    for k, g in grads64.items():
        if g is None:
            continue
        t = max(margin * float(err_ref32[k]), RULE * float(g.abs().max()))
        if k.endswith('weight_g') or k.endswith('weight_v'):
            p = k[:-len('weight_g')]
            bg, bv = weight_norm_bounds(d64(state[p + 'weight_g']), d64(state[p + 'weight_v']), dw64[p])
            t = t + float((bg if k.endswith('weight_g') else bv).max())
        tol[k] = t
    return tol


# ---- operators with their bounds (float64, exact operands) -----------------------------------------------------------------------------------
def gate_factors(a):
    th, sg = torch.tanh(a[:, :RES]), torch.sigmoid(a[:, RES:])
    return th, sg


def gate_backward(dxp, dS, a, wo, wsk):
    """-> (da [B][128][L], bound).  dxp None: the last block (no residual half)."""
    dz = torch.einsum('oi,bot->bit', wsk[:, :, 0], dS)
    ab = torch.einsum('oi,bot->bit', wsk[:, :, 0].abs(), dS.abs())
    if dxp is not None:
        dz = dz + torch.einsum('oi,bot->bit', wo[:, :, 0], S * dxp)
        ab = ab + torch.einsum('oi,bot->bit', wo[:, :, 0].abs(), (S * dxp).abs())
    th, sg = gate_factors(a)
    f = torch.cat([sg * (1 - th * th), th * sg * (1 - sg)], 1)
    dz2, ab2 = torch.cat([dz, dz], 1), torch.cat([ab, ab], 1)
    da = dz2 * f
    return da, RULE * ab2 * f.abs() + E_GATE * dz2.abs() + 4 * U * da.abs()


def conv_backward(da, dxp, wc, wa, dil, dc_prev=None):
    """-> (dx, bound), (dC, bound)"""
    dx = F.conv_transpose1d(da, wc, padding=dil, dilation=dil)
    bx = F.conv_transpose1d(da.abs(), wc.abs(), padding=dil, dilation=dil)
    if dxp is not None:
        dx, bx = dx + S * dxp, bx + (S * dxp).abs()
    if wa is None:
        return (dx, RULE * bx), (None, None)
    dc = torch.einsum('oa,bot->bat', wa[:, :, 0], da)
    bc = torch.einsum('oa,bot->bat', wa[:, :, 0].abs(), da.abs())
    if dc_prev is not None:
        dc, bc = dc + dc_prev, bc + dc_prev.abs()
    return (dx, RULE * bx), (dc, RULE * bc)


def _taps(da, x, dil):
    T = x.shape[2]
    xp = F.pad(x, (dil, dil))
    return torch.cat([torch.einsum('bot,bit->oi', da, xp[:, :, k * dil:k * dil + T]) for k in range(3)], 1)


def wgrad_conv(da, x, cond, dil):
    """-> (dW [128][192 + aux] with columns tap * 64 + ci then the aux channels, bound), (db, bound)"""
    dw, bw = _taps(da, x, dil), _taps(da.abs(), x.abs(), dil)
    if cond is not None:
        dw = torch.cat([dw, torch.einsum('bot,bat->oa', da, cond)], 1)
        bw = torch.cat([bw, torch.einsum('bot,bat->oa', da.abs(), cond.abs())], 1)
    return (dw, RULE * bw), (da.sum((0, 2)), RULE * da.abs().sum((0, 2)))


def wgrad_out(dxp, dS, a):
    """-> (dW [128][64]: rows 0..63 conv1x1_out (zeros without dxp), 64..127 conv1x1_skip, bound), (db, bound)"""
    th, sg = gate_factors(a)
    z = th * sg
    G = torch.cat([S * dxp if dxp is not None else torch.zeros_like(dS), dS], 1)
    dw = torch.einsum('bot,bit->oi', G, z)
    bw = RULE * torch.einsum('bot,bit->oi', G.abs(), z.abs()) + E_GATE * G.abs().sum((0, 2))[:, None]
    return (dw, bw), (G.sum((0, 2)), RULE * G.abs().sum((0, 2)))


def wgrad_relu(g, saved):
    r = torch.relu(saved)
    return (torch.einsum('bot,bit->oi', g, r), RULE * torch.einsum('bot,bit->oi', g.abs(), r)), (g.sum((0, 2)), RULE * g.abs().sum((0, 2)))


def upsample_backward(g, inp, filt, scale):
    """-> (din, bound), (dfilt [2 scale + 1], bound)"""
    def grads(g_, i_, f_):
        i_, f_ = i_.clone().requires_grad_(True), f_.clone().requires_grad_(True)
        return torch.autograd.grad(upsample(i_, f_, scale), (i_, f_), g_)
    di, df = grads(g, inp, filt)
    bi, bf = grads(g.abs(), inp.abs(), filt.abs())
    return (di, RULE * bi), (df.reshape(-1), RULE * bf.reshape(-1))


def convin_wgrad(g, c):
    """conv_in (no padding): dw[co][ci][k] = sum_b sum_t g[b][co][t] c[b][ci][t + k]"""
    L = g.shape[2]
    K = c.shape[2] - L + 1
    dw = torch.stack([torch.einsum('bot,bit->oi', g, c[:, :, k:k + L]) for k in range(K)], 2)
    bw = torch.stack([torch.einsum('bot,bit->oi', g.abs(), c[:, :, k:k + L].abs()) for k in range(K)], 2)
    return dw, RULE * bw


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pwg_train_ref.npz')


def fixture():
    """tests/golden/pwg_train_ref.npz (tools/make_golden_pwg_train.py) -> dict(cfg, state, x, c, target, out, grads, none_keys, err, err_out); the
    state is synth_state(..., 20240612) rounded to float16 by the tool (to keep the file below 1 MiB), stored as float16 and returned as float32:
    synth_state alone does not reproduce it"""
    z = np.load(FIXTURE)
    pick = lambda pre: {k[len(pre):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(pre)}   # noqa: E731
    meta = json.loads(str(z['meta_json']))
    return dict(cfg=config(**meta['cfg']), none_keys=meta['none_keys'], state=pick('state/'), grads=pick('grad/'),
                err={k: float(v) for k, v in pick('err/').items()}, err_out=float(z['err_out']), x=torch.from_numpy(z['x']),
                c=torch.from_numpy(z['c']), target=torch.from_numpy(z['target']), out=torch.from_numpy(z['out']))


def mse_to(target):
    return lambda y: torch.mean((y - target.to(y.device, y.dtype)) ** 2)
