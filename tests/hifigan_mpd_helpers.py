"""Test infrastructure of the HiFi-GAN period discriminator (include/dsv.h, section "HiFi-GAN period discriminator"): float64 restatements on the
CPU, written from the reference's lines IN THE REFERENCE'S LAYOUT (modules/hifigan/hifigan.py:181-250: DiscriminatorP - F.pad(x, (0, n_pad),
'reflect'), view(b, c, t // period, period), five Conv2d((5, 1), (3, 1) x 4 then 1, padding (2, 0)) + F.leaky_relu(x, 0.1) and conv_post (3, 1), every
post-activation and the last output appended to fmap, flatten; MultiPeriodDiscriminator - periods 2, 3, 5, 7, 11, d(y) then d(y_hat);
feature_loss :328-334; the LSGAN losses :337-365) - F.pad, view and F.conv2d, independent of how the product lays its rows out.

The bounds are built by THE RULE of tests/pwg_disc_helpers.py (imported, not re-chosen): an fp32 sum of products may differ from float64 by at
most RULE = 16 u sum|term| element-wise; operand bounds propagate through the same sum as in tests/hifigan_disc_helpers.py, whose loss and
cotangent pieces are imported.  Where a test hands in the device's saved activations they are exact operands and every layer's bound starts
afresh; chained through a whole discriminator the bounds are worst cases that grow by some tens per layer (see hifigan_disc_helpers) and a
comparison needs a closeness check beside them."""
import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.hifigan_disc_helpers import (feature_loss64, l1_cotangents, lsgan64, lsgan_ct, sample_index, synth_state, twin_losses,  # noqa: F401
                                        weight_norm_bound)
from tests.pwg_disc_helpers import RULE, U, d64, leaky, mask_of, weight_norm64, weight_norm_grads64  # noqa: F401

SLOPE = 0.1
PERIODS = (2, 3, 5, 7, 11)
# (Ci, Co, K, stride), padding (K - 1) / 2 along H: hifigan.py:193-200
LAYERS = ((1, 32, 5, 3), (32, 128, 5, 3), (128, 512, 5, 3), (512, 1024, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1))
N = len(LAYERS)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hifigan_mpd_ref.npz')
# THE SEED.  At T = 300 the sixty maps hold about a million activations and every seeded state puts some pre-activation, or some difference r - g,
# within float32 noise of zero: a LeakyReLU mask or an L1 sign that flips there moves a gradient row of a layer with H = 1 by percent, for ANY
# float32 implementation.  Of the seeds 20241020 .. 20241059 this one keeps the smallest |pre-activation| and |r - g| furthest from zero in units
# of the float32 CPU twin's own deviation on the same map (kink_and_tie_margin below: 0.62; the other seeds 0.04 .. 0.45) - chosen from the twin and
# the float64 restatement alone, never from the code under test.
FIXTURE_SEED, FIXTURE_B, FIXTURE_T, FIXTURE_SAMPLES = 20241037, 1, 300, 256


def geom(l):
    _, _, k, s = LAYERS[l]
    return s, (k - 1) // 2


def heights(T, p):
    """[H0, H1, .., H6]: H0 the folded height, H_{l+1} the output height of layer l"""
    hs = [-(-T // p)]
    for l in range(N):
        _, _, k, s = LAYERS[l]
        hs.append((hs[-1] + 2 * ((k - 1) // 2) - k) // s + 1)
    return hs


def fold64(x, p):
    """hifigan.py:211-217: [B][1][T] -> [B][1][H0][p]"""
    b, c, t = x.shape
    if t % p != 0:
        n_pad = p - t % p
        x = F.pad(x, (0, n_pad), 'reflect')
        t = t + n_pad
    return x.view(b, c, t // p, p)


def fold_backward64(g, T, p):
    """the fold's adjoint: [B][1][H0][p] -> [B][1][T]"""
    x = torch.zeros(g.shape[0], 1, T, dtype=g.dtype, requires_grad=True)
    fold64(x, p).backward(g)
    return x.grad


def fold_backward_bound(g, e_g, T, p):
    y = fold_backward64(g, T, p)
    e = U * fold_backward64(g.abs(), T, p)                      # at most one addition per sample
    if e_g is not None:
        e = e + fold_backward64(e_g, T, p)
    return y, e


# ---- one convolution and its gradients, with bounds -------------------------------------------------------------------------------------------
def conv_g(x, w, b, s, pad):
    return F.conv2d(x, w, b, stride=(s, 1), padding=(pad, 0))


def conv_bound(x, w, b, ge, e_in=None, e_w=None):
    """(W x + b in float64, RULE (|W| |x| + |b|) [+ |W| e_in + e_w |x| + e_w e_in])"""
    y = conv_g(x, w, b, *ge)
    bound = RULE * conv_g(x.abs(), w.abs(), None if b is None else b.abs(), *ge)
    if e_in is not None:
        bound = bound + conv_g(e_in, w.abs(), None, *ge)
    if e_w is not None:
        bound = bound + conv_g(x.abs() if e_in is None else x.abs() + e_in, e_w, None, *ge)
    return y, bound


def _convT(G, w, H_in, ge):
    s, pad = ge
    opad = H_in - ((G.shape[2] - 1) * s - 2 * pad + w.shape[2])
    return F.conv_transpose2d(G, w, None, stride=(s, 1), padding=(pad, 0), output_padding=(opad, 0))


def dgrad_bound(G, e_G, w, H_in, ge, e_w=None):
    """(W^T * G in float64, RULE |W|^T |G| [+ |W|^T e_G + e_w^T (|G| + e_G)])"""
    y = _convT(G, w, H_in, ge)
    bound = RULE * _convT(G.abs(), w.abs(), H_in, ge)
    if e_G is not None:
        bound = bound + _convT(e_G, w.abs(), H_in, ge)
    if e_w is not None:
        bound = bound + _convT(G.abs() if e_G is None else G.abs() + e_G, e_w, H_in, ge)
    return y, bound


def _corr(G, a, wshape, ge):
    """dW[co][ci][k][0] = sum_b sum_h sum_w G[b][co][h][w] a[b][ci][h s + k - pad][w]"""
    s, pad = ge
    return torch.nn.grad.conv2d_weight(a, wshape, G, stride=(s, 1), padding=(pad, 0))


def wgrad_bound(G, e_G, a, e_a, wshape, ge):
    """(dW, bound), (db, bound)"""
    dw, db = _corr(G, a, wshape, ge), G.sum((0, 2, 3))
    bw, bb = RULE * _corr(G.abs(), a.abs(), wshape, ge), RULE * G.abs().sum((0, 2, 3))
    if e_G is not None:
        bw = bw + _corr(e_G, a.abs(), wshape, ge)
        bb = bb + e_G.sum((0, 2, 3))
    if e_a is not None:
        bw = bw + _corr(G.abs() if e_G is None else G.abs() + e_G, e_a, wshape, ge)
    return (dw, bw), (db, bb)


# ---- the stack ----------------------------------------------------------------------------------------------------------------------------------
def forward64(x, p, ws, bs, slope=SLOPE, inputs=None, e_ws=None):
    """DiscriminatorP.forward in float64 -> dict(xf, fmap, e_fmap): the folded input, the six feature maps and their bounds (fmap[5] is the output
    before flatten).  inputs None: the bound propagates from x (exact: the fold copies); inputs = the device's six feature maps (float64): layer
    l >= 1 reads inputs[l - 1] as an exact operand.  e_ws: bounds of the weights (the normalisation computed in float32), or None."""
    xf = fold64(x, p)
    h, e = xf, None
    fmap, e_fmap = [], []
    for l in range(N):
        if inputs is not None and l > 0:
            h, e = inputs[l - 1], None
        pre, eb = conv_bound(h, ws[l], bs[l], geom(l), e, None if e_ws is None else e_ws[l])
        if l < N - 1:
            a = leaky(pre, slope)
            eb = eb + U * a.abs()                               # the product with the slope rounds once more; the activation is 1-Lipschitz
        else:
            a = pre
        fmap.append(a); e_fmap.append(eb)
        h, e = a, eb
    return dict(xf=xf, fmap=fmap, e_fmap=e_fmap)


def backward64(g_out, g_fmap, xf, T, p, ws, acts, slope=SLOPE, e_acts=None, e_ws=None, e_g_fmap=None, e_g_out=None):
    """Backward of the stack in float64.  g_out [B][H p] or None, g_fmap: six cotangents (None where absent) with bounds e_g_fmap / e_g_out (None:
    exact).  acts: the six feature maps, used BOTH as the masks and as the weight gradients' operands (the device's: e_acts None; or forward64's
    own with their bounds).  -> dict(dw=[(value, bound)] * 6, db=[...], G=[gradient with respect to layer l's pre-activation, (value, bound)],
    dxf=(value, bound) [B][1][H0][p], dx=(value, bound) [B][1][T])"""
    ea = (lambda i: None) if e_acts is None else (lambda i: e_acts[i])
    eg = (lambda i: None) if e_g_fmap is None else (lambda i: e_g_fmap[i])
    G, e_G, n_add = torch.zeros_like(acts[N - 1]), torch.zeros_like(acts[N - 1]), 0
    for t, et in ((None if g_out is None else g_out.reshape(acts[N - 1].shape), None if e_g_out is None else e_g_out.reshape(acts[N - 1].shape)),
                  (g_fmap[N - 1], eg(N - 1))):
        if t is not None:
            G, n_add = G + t, n_add + 1
            if et is not None:
                e_G = e_G + et
    if n_add == 2:
        e_G = e_G + U * G.abs()
    dws, dbs, Gs = [None] * N, [None] * N, [None] * N
    for l in range(N - 1, -1, -1):
        Gs[l] = (G, e_G)
        a_in, e_a = (acts[l - 1], ea(l - 1)) if l > 0 else (xf, None)
        dws[l], dbs[l] = wgrad_bound(G, e_G, a_in, e_a, ws[l].shape, geom(l))
        D, e_D = dgrad_bound(G, e_G, ws[l], a_in.shape[2], geom(l), None if e_ws is None else e_ws[l])
        if l == 0:
            return dict(dw=dws, db=dbs, G=Gs, dxf=(D, e_D), dx=fold_backward_bound(D, e_D, T, p))
        if g_fmap[l - 1] is not None:
            D = D + g_fmap[l - 1]
            e_D = e_D + U * D.abs() + (0 if eg(l - 1) is None else eg(l - 1))
        m = mask_of(acts[l - 1], slope)
        G = D * m
        e_G = e_D * m + U * G.abs()
        if ea(l - 1) is not None:                               # a sign within the activation's own bound may be the other one in float32
            e_G = e_G + torch.where(acts[l - 1].abs() <= ea(l - 1), (1.0 - slope) * (D.abs() + e_D), torch.zeros_like(D))


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------
def prefixes(i):
    return [f'discriminators.{i}.convs.{l}.' for l in range(N - 1)] + [f'discriminators.{i}.conv_post.']


def module_shapes():
    """state-dict keys and shapes of the reference's MultiPeriodDiscriminator (recorded in the fixture; restated here): 90 entries"""
    out = {}
    for i in range(len(PERIODS)):
        for l, pre in enumerate(prefixes(i)):
            ci, co, k, _ = LAYERS[l]
            out[pre + 'bias'] = (co,)
            out[pre + 'weight_g'] = (co, 1, 1, 1)
            out[pre + 'weight_v'] = (co, ci, k, 1)
    return out


def synth_plain(seed, slope=SLOPE):
    """plain float32 weights [Co][Ci][K][1] and biases of one DiscriminatorP with O(1) activations: rows of norm about the gain"""
    gen = torch.Generator().manual_seed(seed)
    gain = (2.0 / (1.0 + slope * slope)) ** 0.5
    ws, bs = [], []
    for ci, co, k, _ in LAYERS:
        w = torch.randn(co, ci, k, 1, generator=gen)
        ws.append(gain * (0.8 + 0.4 * torch.rand(co, 1, 1, 1, generator=gen)) * w / w.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1))
        bs.append(0.1 * torch.randn(co, generator=gen))
    return ws, bs


def disc_weights(state, i):
    """effective float64 weights of discriminator i from a float64 state in either form -> dict(ws, e_ws, bs)"""
    ws, e_ws, bs = [], [], []
    for pre in prefixes(i):
        bs.append(state[pre + 'bias'])
        if pre + 'weight' in state:
            ws.append(state[pre + 'weight']); e_ws.append(torch.zeros_like(state[pre + 'weight']))
        else:
            w, e = weight_norm_bound(state[pre + 'weight_g'], state[pre + 'weight_v'])
            ws.append(w); e_ws.append(e)
    return dict(ws=ws, e_ws=e_ws, bs=bs)


def mpd_forward64(state, y, y_hat):
    """MultiPeriodDiscriminator.forward in float64 with bounds -> dict(r, g: per discriminator forward64 results + 'w' (disc_weights))"""
    st = {k: d64(v) for k, v in state.items()}
    out = {'r': [], 'g': []}
    for i, p in enumerate(PERIODS):
        wt = disc_weights(st, i)
        for s, x in (('r', d64(y)), ('g', d64(y_hat))):
            f = forward64(x, p, wt['ws'], wt['bs'], e_ws=wt['e_ws'])
            f['w'] = wt
            out[s].append(f)
    return out


def mpd_losses64(fw):
    """(feature_loss, generator_loss, r_loss, g_loss) of hifigan.py:328-365 from mpd_forward64's result, float64"""
    n = len(PERIODS)
    fl, _ = feature_loss64([f['fmap'] for f in fw['r']], [f['fmap'] for f in fw['g']])
    gen = sum(lsgan64(f['fmap'][N - 1], 1.0) for f in fw['g']) / n
    rl = sum(lsgan64(f['fmap'][N - 1], 1.0) for f in fw['r']) / n
    gl = sum(lsgan64(f['fmap'][N - 1], 0.0) for f in fw['g']) / n
    return fl, gen, rl, gl


def mpd_backward64(fw, state, T, w_fm=1.0, w_gen=1.0, w_r=1.0, w_g=1.0):
    """Gradients of L = w_fm feature_loss + w_gen generator_loss + w_r r_loss + w_g g_loss with bounds -> dict(grads {key: (value, bound)},
    dy_hat (value, bound))"""
    st = {k: d64(v) for k, v in state.items()}
    n = len(PERIODS)
    grads, dyh, e_dyh = {}, None, None
    for i, p in enumerate(PERIODS):
        per_side = {}
        for s in ('r', 'g'):
            f, o = fw[s][i], fw['g' if s == 'r' else 'r'][i]
            cts, e_cts = [], []
            for l in range(N):
                r_, g_ = (f, o) if s == 'r' else (o, f)
                ct, e = l1_cotangents(r_['fmap'][l], g_['fmap'][l], r_['e_fmap'][l], g_['e_fmap'][l], scale=2.0 * w_fm)
                cts.append(ct if s == 'r' else -ct); e_cts.append(e)
            pp = f['fmap'][N - 1]
            if s == 'r':
                go, e_go = lsgan_ct(pp, 1.0, w_r / n, f['e_fmap'][N - 1])
            else:
                g1, e1 = lsgan_ct(pp, 1.0, w_gen / n, f['e_fmap'][N - 1])
                g0, e0 = lsgan_ct(pp, 0.0, w_g / n, f['e_fmap'][N - 1])
                go, e_go = g1 + g0, e1 + e0 + U * (g1 + g0).abs()
            per_side[s] = backward64(go.reshape(pp.shape[0], -1), cts, f['xf'], T, p, f['w']['ws'], f['fmap'], e_acts=f['e_fmap'], e_ws=f['w']['e_ws'],
                                     e_g_fmap=e_cts, e_g_out=e_go.reshape(pp.shape[0], -1))
        for l, pre in enumerate(prefixes(i)):
            for s in ('r', 'g'):
                bw = per_side[s]
                (dw, e_dw), (db, e_db) = bw['dw'][l], bw['db'][l]
                if pre + 'weight' in st:
                    part = {pre + 'weight': (dw, e_dw), pre + 'bias': (db, e_db)}
                else:
                    (gg, e_gg), (gv, e_gv) = weight_norm_grads64(st[pre + 'weight_g'], st[pre + 'weight_v'], dw, e_dw)
                    part = {pre + 'weight_g': (gg, e_gg), pre + 'weight_v': (gv, e_gv), pre + 'bias': (db, e_db)}
                for k, (v, e) in part.items():
                    if k in grads:
                        v0, e0 = grads[k]
                        grads[k] = (v0 + v, e0 + e + U * (v0 + v).abs())
                    else:
                        grads[k] = (v, e)
        d, e = per_side['g']['dx']
        dyh, e_dyh = (d, e) if dyh is None else (dyh + d, e_dyh + e + U * (dyh + d).abs())
    return dict(grads=grads, dy_hat=(dyh, e_dyh))


# ---- the module as torch modules (the twin) -------------------------------------------------------------------------------------------------------
class TwinP(nn.Module):
    """hifigan.py:181-227 restated: torch Conv2d under torch's own weight_norm"""

    def __init__(self, period):
        super().__init__()
        from torch.nn.utils import weight_norm
        self.period = period
        mods = [weight_norm(nn.Conv2d(ci, co, (k, 1), (s, 1), padding=((k - 1) // 2, 0))) for ci, co, k, s in LAYERS]
        self.convs = nn.ModuleList(mods[:-1])
        self.conv_post = mods[-1]

    def forward(self, x, mel=None):
        fmap = []
        x = fold64(x, self.period)
        for m in self.convs:
            x = F.leaky_relu(m(x), SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class TwinMPD(nn.Module):
    """hifigan.py:230-250 restated"""

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([TwinP(p) for p in PERIODS])

    def forward(self, y, y_hat, mel=None):
        rs, gs, frs, fgs = [], [], [], []
        for d in self.discriminators:
            r, fr = d(y)
            g, fg = d(y_hat)
            rs.append(r); gs.append(g); frs.append(fr); fgs.append(fg)
        return rs, gs, frs, fgs


def kink_and_tie_margin(fmap_r, fmap_g, fmap_r32, fmap_g32, slope=SLOPE):
    """the smallest |pre-activation| and |r - g| over lists of float64 maps (per discriminator), each in units of the largest deviation of the
    float32 maps from them on the same map (both deviations for a difference): below 1 a flip is possible, and the larger the less likely"""
    worst = float('inf')
    for dr, dg, dr32, dg32 in zip(fmap_r, fmap_g, fmap_r32, fmap_g32):
        for l in range(N):
            nr = float((dr32[l].double() - dr[l]).abs().max())
            ng = float((dg32[l].double() - dg[l]).abs().max())
            if l < N - 1:
                for a, n in ((dr[l], nr), (dg[l], ng)):
                    pre = torch.where(a > 0, a, a / slope)
                    worst = min(worst, float(pre.abs().min()) / n)
            worst = min(worst, float((dr[l] - dg[l]).abs().min()) / (nr + ng))
    return worst


# ---- fixture ---------------------------------------------------------------------------------------------------------------------------------------
def fixture():
    """tests/golden/hifigan_mpd_ref.npz (tools/make_golden_hifigan_mpd.py) -> dict of arrays; 'meta' is the decoded meta_json"""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files if k != 'meta_json'}
    out['meta'] = json.loads(str(z['meta_json']))
    return out


def fixture_inputs():
    """(state, y, y_hat) of the fixture's recipe: the seeded state rounded to float16 values (held in float32), seeded waveforms"""
    state = {k: v.half().float() for k, v in synth_state(module_shapes(), FIXTURE_SEED, SLOPE).items()}
    gen = torch.Generator().manual_seed(FIXTURE_SEED + 1)
    y = 0.5 * torch.randn(FIXTURE_B, 1, FIXTURE_T, generator=gen)
    y_hat = y + 0.3 * torch.randn(FIXTURE_B, 1, FIXTURE_T, generator=gen)
    return state, y, y_hat
