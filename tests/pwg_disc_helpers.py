"""Test infrastructure of the ParallelWaveGAN discriminator (include/dsv.h, section "PWG discriminator"): float64 restatements on the CPU, written
from the reference's lines (modules/parallel_wavegan/models/parallel_wavegan.py:207-300: Conv1d(kernel 3, padding = dilation) + LeakyReLU(inplace),
dilation 1, 1, 2, ..., layers - 2, 1; modules/hifigan/hifigan.py:337-365) and independent of the product code, and the error rule the tests
apply to them.

THE RULE.  u = 2^-24.  A convolution output, or a gradient that is an fp32 sum of products, may differ from float64 by at most
16 u sum|term| element-wise, sum|term| being the same sum over absolute values in float64.  Where the operands of a sum carry an error bound E of
their own (a chain of layers), the bound propagates through the same sum: |W| * E for a convolution, sum E_G |a| + sum |G| E_a + sum E_G E_a for a
weight gradient.  Every function below returns (value, bound) pairs built this way; nothing is taken from the code under test.

The LeakyReLU here takes its mask from OUTSIDE when one is given (m = 1 where the given post-activation > 0, else slope - the in-place
activation's autograd rule: an output of exactly 0 takes the slope)."""
import json

import torch
import torch.nn.functional as F

U = 2.0 ** -24
RULE = 16.0 * U
C = 64


def dilation_of(i, n):
    """dilation of conv i of an n-conv stack (parallel_wavegan.py:244-261)"""
    return 1 if i == 0 or i == n - 1 else i


def d64(t):
    return t.detach().to('cpu', torch.float64)


def conv(x, w, b, dil):
    return F.conv1d(x, w, b, padding=dil, dilation=dil)


def conv_bound(x, w, b, dil, e_in=None):
    """(W x + b in float64, 16 u (|W| |x| + |b|) [+ |W| e_in])"""
    y = conv(x, w, b, dil)
    bound = RULE * conv(x.abs(), w.abs(), None if b is None else b.abs(), dil)
    if e_in is not None:
        bound = bound + conv(e_in, w.abs(), None, dil)
    return y, bound


def leaky(pre, slope):
    return torch.where(pre > 0, pre, pre * slope)


def mask_of(a, slope):
    """the in-place LeakyReLU's derivative from its OUTPUT"""
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))


def forward64(x, ws, bs, slope, inputs=None):
    """The stack in float64.  inputs None: every layer reads the activation computed here and the bound propagates from x (exact);
    inputs = [a_0 ... a_{n-2}] (the device's saved activations, float64): layer l >= 1 reads inputs[l - 1] as an exact operand - the bound of
    every layer is then the rule applied to the device's own operands.  -> dict(pre, act, e_act (bounds of act), p, e_p)"""
    n = len(ws)
    h, e = x, None
    pres, acts, e_acts = [], [], []
    for i in range(n - 1):
        if inputs is not None and i > 0:
            h, e = inputs[i - 1], None
        pre, eb = conv_bound(h, ws[i], bs[i], dilation_of(i, n), e)
        a = leaky(pre, slope)
        eb = eb + U * a.abs()                                   # the product with the slope rounds once more; the activation is 1-Lipschitz
        pres.append(pre); acts.append(a); e_acts.append(eb)
        h, e = a, eb
    if inputs is not None:
        h, e = inputs[n - 2], None
    p, e_p = conv_bound(h, ws[n - 1], bs[n - 1], 1, e)
    return dict(pre=pres, act=acts, e_act=e_acts, p=p, e_p=e_p)


def dgrad_bound(G, e_G, w, dil):
    """((W^T * G) in float64, 16 u |W|^T * |G| + |W|^T * e_G)"""
    y = F.conv_transpose1d(G, w, padding=dil, dilation=dil)
    bound = RULE * F.conv_transpose1d(G.abs(), w.abs(), padding=dil, dilation=dil)
    if e_G is not None:
        bound = bound + F.conv_transpose1d(e_G, w.abs(), padding=dil, dilation=dil)
    return y, bound


def _corr(G, a, dil):
    """sum_b sum_t G[b][co][t] a[b][ci][t + (k - 1) dil] -> [co][ci][3]"""
    T = G.shape[2]
    ap = F.pad(a, (dil, dil))
    return torch.stack([torch.einsum('bot,bit->oi', G, ap[:, :, k * dil:k * dil + T]) for k in range(3)], 2)


def wgrad_bound(G, e_G, a, e_a, dil):
    """(dW, bound), (db, bound)"""
    dw, db = _corr(G, a, dil), G.sum((0, 2))
    bw, bb = RULE * _corr(G.abs(), a.abs(), dil), RULE * G.abs().sum((0, 2))
    if e_G is not None:
        bw = bw + _corr(e_G, a.abs(), dil)
        bb = bb + e_G.sum((0, 2))
    if e_a is not None:
        bw = bw + _corr(G.abs(), e_a, dil)
        if e_G is not None:
            bw = bw + _corr(e_G, e_a, dil)
    return (dw, bw), (db, bb)


def backward64(gp, e_gp, x, ws, acts, slope, e_acts=None):
    """Backward of the stack in float64 from gp = dL/dp [B][1][T] with bound e_gp.  acts: the post-activations used BOTH as the masks and as the
    weight gradients' operands (the device's saved ones: e_acts None, they are exact operands; or forward64's own with their bounds).
    -> dict(dw=[(value, bound)] * n, db=[...], dx=(value, bound))"""
    n = len(ws)
    ea = (lambda i: None) if e_acts is None else (lambda i: e_acts[i])
    dws, dbs = [None] * n, [None] * n
    dws[n - 1], dbs[n - 1] = wgrad_bound(gp, e_gp, acts[n - 2], ea(n - 2), 1)
    G, e_G = dgrad_bound(gp, e_gp, ws[n - 1], 1)
    for l in range(n - 2, -1, -1):
        m = mask_of(acts[l], slope)
        G, e_G = G * m, e_G * m + U * (G * m).abs()
        if l == 0:
            break
        dws[l], dbs[l] = wgrad_bound(G, e_G, acts[l - 1], ea(l - 1), dilation_of(l, n))
        G, e_G = dgrad_bound(G, e_G, ws[l], dilation_of(l, n))
    dws[0], dbs[0] = wgrad_bound(G, e_G, x, None, 1)
    return dict(dw=dws, db=dbs, dx=dgrad_bound(G, e_G, ws[0], 1))


def lsgan64(d, target):
    return ((d64(d) - target) ** 2).mean()


def generator_gp(p, e_p):
    """d mean((1 - p)^2) / dp and its bound (two roundings of its own)"""
    gp = 2.0 * (p - 1.0) / p.numel()
    e = 2.0 * U * gp.abs()
    if e_p is not None:
        e = e + 2.0 * e_p / p.numel()
    return gp, e


def weight_norm64(g, v):
    return g * v / v.flatten(1).norm(dim=1).reshape(g.shape)


def weight_norm_grads64(g, v, dw, e_dw=None):
    """gradients of w = g v / ||v|| (torch.nn.utils.weight_norm, dim 0) given dL/dw, in float64 by autograd, with the rule's bound:
    16 u times the sums of absolute terms, plus the same linear map in absolute value applied to e_dw."""
    g, v = g.clone().requires_grad_(True), v.clone().requires_grad_(True)
    weight_norm64(g, v).backward(dw)
    nrm = v.detach().flatten(1).norm(dim=1).reshape(g.shape)
    va, ga = v.detach().abs(), g.detach().abs()

    def absmap(d):
        s = (d * va).flatten(1).sum(1).reshape(g.shape)
        return s / nrm, ga / nrm * d + ga * s / nrm ** 3 * va
    bg, bv = absmap(dw.abs())
    bg, bv = RULE * bg, RULE * bv
    if e_dw is not None:
        eg, ev = absmap(e_dw)
        bg, bv = bg + eg, bv + ev
    return (g.grad, bg), (v.grad, bv)


# ---- seeded states ---------------------------------------------------------------------------------------------------------------------------
def module_shapes(layers=10, bias=True, weight_norm=True):
    """state-dict keys and shapes of the reference module (recorded in the fixture for the default 10 layers; restated here for the others)"""
    out = {}
    for i in range(layers):
        co, ci = (1 if i == layers - 1 else C), (1 if i == 0 else C)
        pre = f'conv_layers.{2 * i}.'
        if bias:
            out[pre + 'bias'] = (co,)
        if weight_norm:
            out[pre + 'weight_g'] = (co, 1, 1)
            out[pre + 'weight_v'] = (co, ci, 3)
        else:
            out[pre + 'weight'] = (co, ci, 3)
    return out


def synth_state(shapes, seed, slope=0.2):
    """Seeded parameters that keep the activations O(1) through the stack: every output row of a plain weight has norm about
    sqrt(2 / (1 + slope^2)) (the variance a LeakyReLU loses), biases 0.1 N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    gain = (2.0 / (1.0 + slope * slope)) ** 0.5
    st = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith('bias'):
            st[k] = 0.1 * torch.randn(shp, generator=gen)
        elif k.endswith('weight_g'):
            st[k] = gain * (0.8 + 0.4 * torch.rand(shp, generator=gen))
        elif k.endswith('weight_v'):
            st[k] = torch.randn(shp, generator=gen)
        else:                                                   # plain weight: rows of norm ~ gain
            w = torch.randn(shp, generator=gen)
            st[k] = gain * (0.8 + 0.4 * torch.rand(shp[0], 1, 1, generator=gen)) * w / w.flatten(1).norm(dim=1).reshape(-1, 1, 1)
    return st


def plain_params(state, layers):
    """float64 plain weights and biases (None where absent) of a state dict in either form"""
    ws, bs = [], []
    for i in range(layers):
        pre = f'conv_layers.{2 * i}.'
        if pre + 'weight' in state:
            ws.append(d64(state[pre + 'weight']))
        else:
            ws.append(weight_norm64(d64(state[pre + 'weight_g']), d64(state[pre + 'weight_v'])))
        bs.append(d64(state[pre + 'bias']) if pre + 'bias' in state else None)
    return ws, bs


def fixture():
    """tests/golden/pwg_disc_ref.npz (tools/make_golden_pwg_disc.py) -> dict(state, x, out, dx, grads, keys)"""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pwg_disc_ref.npz'))
    state = {k[len('state/'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('state/')}
    grads = {k[len('grad/'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('grad/')}
    return dict(state=state, grads=grads, x=torch.from_numpy(z['x']), out=torch.from_numpy(z['out']), dx=torch.from_numpy(z['dx']),
                layers=int(z['layers']), slope=float(z['slope']), keys=json.loads(str(z['keys_json'])))
