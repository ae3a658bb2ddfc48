"""Test infrastructure of the HiFi-GAN scale discriminator (include/dsv.h, section "HiFi-GAN scale discriminator"): float64 restatements on the CPU,
written from the reference's lines (modules/hifigan/hifigan.py:253-334: DiscriminatorS - seven Conv1d + F.leaky_relu(x, 0.1) and conv_post, every
post-activation and the last output appended to fmap; MultiScaleDiscriminator - three of them, the first under spectral_norm, the others under
weight_norm, AvgPool1d(4, 2, padding=1) applied cumulatively in front of the second and third; feature_loss; :337-365 the LSGAN losses) and
independent of the product code, with the error bounds the tests apply to them.

The bounds are built by THE RULE of tests/pwg_disc_helpers.py (imported, not re-chosen): an fp32 sum of products may differ from float64 by at
most RULE = 16 u sum|term| element-wise; operand bounds propagate through the same sum - |W| * E (and E_W * |x|) for a convolution,
sum E_G |a| + sum |G| E_a + sum E_G E_a for a weight gradient.  Where a test hands in the device's saved activations they are exact operands.
A single rounding (an addition, a product with the slope or the mask, a division by a constant) adds u |result|.

WHAT THE CHAINED BOUNDS ARE WORTH.  They are worst cases and grow by a factor of some tens per layer.  With the device's activations handed in as
exact operands (forward64(inputs=...), backward64(e_acts=None)) every layer's bound starts afresh and is a few times the observed error - that is
the use they are built for.  Propagated from the input through a whole discriminator (msd_forward64, msd_backward64) they exceed the values
themselves from about the fourth layer on, and every gradient's: there they only say that nothing is outside a worst case, and a comparison needs
a closeness check of its own beside them, as tests/test_hifigan_disc_host.py has."""
import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.pwg_disc_helpers import RULE, U, d64, leaky, mask_of, weight_norm64, weight_norm_grads64  # noqa: F401

SLOPE = 0.1
# (Ci, Co, K, stride, groups), padding (K - 1) / 2: hifigan.py:263-271
LAYERS = ((1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (256, 512, 41, 4, 16), (512, 1024, 41, 4, 16), (1024, 1024, 41, 1, 16),
          (1024, 1024, 5, 1, 1), (1024, 1, 3, 1, 1))
N = len(LAYERS)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hifigan_disc_ref.npz')
FIXTURE_SEED, FIXTURE_B, FIXTURE_T, FIXTURE_SAMPLES, HOP = 20240911, 1, 300, 256, 256


def geom(l):
    ci, co, k, s, g = LAYERS[l]
    return dict(stride=s, padding=(k - 1) // 2, groups=g)


def out_len(L, l):
    _, _, k, s, _ = LAYERS[l]
    return (L + 2 * ((k - 1) // 2) - k) // s + 1


def lengths(T):
    out = []
    for l in range(N):
        T = out_len(T, l)
        out.append(T)
    return out


# ---- one convolution and its gradients, with bounds -------------------------------------------------------------------------------------------
def conv_g(x, w, b, **ge):
    return F.conv1d(x, w, b, **ge)


def conv_bound(x, w, b, ge, e_in=None, e_w=None):
    """(W x + b in float64, RULE (|W| |x| + |b|) [+ |W| e_in + e_w |x| + e_w e_in])"""
    y = conv_g(x, w, b, **ge)
    bound = RULE * conv_g(x.abs(), w.abs(), None if b is None else b.abs(), **ge)
    if e_in is not None:
        bound = bound + conv_g(e_in, w.abs(), None, **ge)
    if e_w is not None:
        bound = bound + conv_g(x.abs() if e_in is None else x.abs() + e_in, e_w, None, **ge)
    return y, bound


def _convT(G, w, L_in, ge):
    k = w.shape[2]
    opad = L_in - ((G.shape[2] - 1) * ge['stride'] - 2 * ge['padding'] + k)
    return F.conv_transpose1d(G, w, None, stride=ge['stride'], padding=ge['padding'], output_padding=opad, groups=ge['groups'])


def dgrad_bound(G, e_G, w, L_in, ge, e_w=None):
    """(W^T * G in float64, RULE |W|^T |G| [+ |W|^T e_G + e_w^T (|G| + e_G)])"""
    y = _convT(G, w, L_in, ge)
    bound = RULE * _convT(G.abs(), w.abs(), L_in, ge)
    if e_G is not None:
        bound = bound + _convT(e_G, w.abs(), L_in, ge)
    if e_w is not None:
        bound = bound + _convT(G.abs() if e_G is None else G.abs() + e_G, e_w, L_in, ge)
    return y, bound


def _corr(G, a, wshape, ge):
    """dW[co][ci][k] = sum_b sum_q G[b][co][q] a[b][grp(co) Ci/g + ci][q s + k - pad]"""
    return torch.nn.grad.conv1d_weight(a, wshape, G, stride=ge['stride'], padding=ge['padding'], groups=ge['groups'])


def wgrad_bound(G, e_G, a, e_a, wshape, ge):
    """(dW, bound), (db, bound)"""
    dw, db = _corr(G, a, wshape, ge), G.sum((0, 2))
    bw, bb = RULE * _corr(G.abs(), a.abs(), wshape, ge), RULE * G.abs().sum((0, 2))
    if e_G is not None:
        bw = bw + _corr(e_G, a.abs(), wshape, ge)
        bb = bb + e_G.sum((0, 2))
    if e_a is not None:
        bw = bw + _corr(G.abs() if e_G is None else G.abs() + e_G, e_a, wshape, ge)
    return (dw, bw), (db, bb)


# ---- the stack ----------------------------------------------------------------------------------------------------------------------------------
def forward64(x, ws, bs, slope=SLOPE, inputs=None, e_ws=None, e_x=None):
    """DiscriminatorS.forward in float64 -> dict(fmap, e_fmap): the eight feature maps and their bounds (fmap[7] is the output before flatten).
    inputs None: the bound propagates from x (bound e_x); inputs = the device's eight feature maps (float64): layer l >= 1 reads inputs[l - 1]
    as an exact operand.  e_ws: bounds of the weights (normalisations computed in float32), or None."""
    h, e = x, e_x
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
    return dict(fmap=fmap, e_fmap=e_fmap)


def backward64(g_out, g_fmap, x, ws, acts, slope=SLOPE, e_acts=None, e_ws=None, e_g_fmap=None, e_g_out=None):
    """Backward of the stack in float64.  g_out [B][L8] or None, g_fmap: eight cotangents (None where absent) with bounds e_g_fmap / e_g_out (None:
    exact).  acts: the eight feature maps, used BOTH as the masks and as the weight gradients' operands (the device's: e_acts None; or forward64's
    own with their bounds).  -> dict(dw=[(value, bound)] * 8, db=[...], dx=(value, bound))"""
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
    dws, dbs = [None] * N, [None] * N
    for l in range(N - 1, -1, -1):
        a_in, e_a = (acts[l - 1], ea(l - 1)) if l > 0 else (x, None)
        dws[l], dbs[l] = wgrad_bound(G, e_G, a_in, e_a, ws[l].shape, geom(l))
        D, e_D = dgrad_bound(G, e_G, ws[l], a_in.shape[2], geom(l), None if e_ws is None else e_ws[l])
        if l == 0:
            return dict(dw=dws, db=dbs, dx=(D, e_D))
        if g_fmap[l - 1] is not None:
            D = D + g_fmap[l - 1]
            e_D = e_D + U * D.abs() + (0 if eg(l - 1) is None else eg(l - 1))
        m = mask_of(acts[l - 1], slope)
        G = D * m
        e_G = e_D * m + U * G.abs()
        if ea(l - 1) is not None:                               # a sign within the activation's own bound may be the other one in float32
            e_G = e_G + torch.where(acts[l - 1].abs() <= ea(l - 1), (1.0 - slope) * (D.abs() + e_D), torch.zeros_like(D))


# ---- pooling, losses ----------------------------------------------------------------------------------------------------------------------------
def pool64(x):
    """AvgPool1d(4, 2, padding=1), count_include_pad: the divisor is always 4"""
    return F.avg_pool1d(x, 4, 2, 1)


def pool_bound(x, e_x=None):
    y = pool64(x)
    e = 4 * U * pool64(x.abs())                                 # three additions and an exact division by 4
    if e_x is not None:
        e = e + pool64(e_x)
    return y, e


def pool_backward64(g, T):
    """the pooling's adjoint: [B][1][T // 2] -> [B][1][T]"""
    x = torch.zeros(g.shape[0], 1, T, dtype=g.dtype, requires_grad=True)
    pool64(x).backward(g)
    return x.grad


def pool_backward_bound(g, e_g, T):
    y = pool_backward64(g, T)
    e = 2 * U * pool_backward64(g.abs(), T)
    if e_g is not None:
        e = e + pool_backward64(e_g, T)
    return y, e


def feature_loss64(fmap_r, fmap_g):
    """hifigan.py:328-334 -> (value, bound); float64 sums on the device, so the bound is the rounding of the 24 means and their sum"""
    loss = 0.0
    for dr, dg in zip(fmap_r, fmap_g):
        for rl, gl in zip(dr, dg):
            loss = loss + torch.mean(torch.abs(rl - gl))
    return loss * 2, 64 * U * float(loss * 2)


def l1_cotangents(r, g, e_r=None, e_g=None, scale=2.0):
    """d (scale mean|r - g|) / dr (the one of g is its negative) and its bound: a sign that the operands' bounds can flip carries 2 |value|"""
    d = r - g
    ct = scale * torch.sign(d) / d.numel()
    e = 2 * U * ct.abs()
    if e_r is not None or e_g is not None:
        slack = (0 if e_r is None else e_r) + (0 if e_g is None else e_g)
        e = torch.where(d.abs() <= slack, torch.full_like(d, 2 * scale / d.numel()), e)
    return ct, e


def lsgan64(d, target):
    return ((d - target) ** 2).mean()


def lsgan_ct(p, target, weight, e_p=None):
    """d (weight mean((p - target)^2)) / dp and its bound"""
    gp = 2.0 * weight * (p - target) / p.numel()
    e = 3.0 * U * gp.abs()
    if e_p is not None:
        e = e + 2.0 * weight * e_p / p.numel()
    return gp, e


# ---- the normalisations -------------------------------------------------------------------------------------------------------------------------
def _normalize(x, eps=1e-12):
    return x / max(float(x.norm()), eps)


def spectral64(w_orig, u, v, power_iteration, e_u=None, e_v=None):
    """torch.nn.utils.spectral_norm's weight (one power iteration in train() mode: v = normalize(W^T u), u = normalize(W v); sigma = u . (W v);
    weight = W / sigma) -> dict(w, e_w, u, v, e_u, e_v, sigma, e_rel): the bounds follow the float32 evaluation by THE RULE."""
    W = w_orig.flatten(1)
    Wa = W.abs()
    e_u = torch.zeros_like(u) if e_u is None else e_u           # bounds of the buffers handed in (an earlier call's iteration)
    e_v = torch.zeros_like(v) if e_v is None else e_v
    if power_iteration:
        x = W.t() @ u
        e_x = RULE * (Wa.t() @ u.abs()) + Wa.t() @ e_u
        v = _normalize(x)
        e_v = e_x / x.norm() + v.abs() * (e_x.norm() / x.norm() + RULE)
        x = W @ v
        e_x = RULE * (Wa @ v.abs()) + Wa @ e_v
        u = _normalize(x)
        e_u = e_x / x.norm() + u.abs() * (e_x.norm() / x.norm() + RULE)
    Wv = W @ v
    sigma = u @ Wv
    e_sigma = RULE * (u.abs() @ (Wa @ v.abs())) + e_u @ Wv.abs() + (u.abs() + e_u) @ (Wa @ e_v)
    e_rel = float(e_sigma / sigma.abs())
    w = w_orig / sigma
    return dict(w=w, e_w=w.abs() * (e_rel + 2 * U), u=u, v=v, e_u=e_u, e_v=e_v, sigma=sigma, e_rel=e_rel)


def spectral_grad64(w_orig, sp, dw, e_dw):
    """gradient of weight = W / (u . W v) with respect to W, u and v held fixed (torch computes them under no_grad), and its bound"""
    W = w_orig.flatten(1)
    sigma, uv = sp['sigma'], torch.outer(sp['u'], sp['v'])
    dot = (dw.flatten(1) * W).sum()
    g = dw.flatten(1) / sigma - dot / sigma ** 2 * uv
    dota = (dw.flatten(1).abs() * W.abs()).sum()
    e = RULE * (dw.flatten(1).abs() / sigma.abs() + dota / sigma ** 2 * uv.abs()) + g.abs() * 2 * sp['e_rel']
    e = e + e_dw.flatten(1) / sigma.abs() + (e_dw.flatten(1) * W.abs()).sum() / sigma ** 2 * uv.abs()
    e = e + dota / sigma ** 2 * (torch.outer(sp['e_u'], sp['v'].abs()) + torch.outer(sp['u'].abs() + sp['e_u'], sp['e_v']))
    return g.reshape(w_orig.shape), e.reshape(w_orig.shape)


def weight_norm_bound(g, v):
    """(g v / ||v||, its float32 bound: the norm's sum by the rule, a square root, a division and a product)"""
    w = weight_norm64(g, v)
    return w, w.abs() * (RULE + 4 * U)


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------
def prefixes(i):
    return [f'discriminators.{i}.convs.{l}.' for l in range(N - 1)] + [f'discriminators.{i}.conv_post.']


def module_shapes():
    """state-dict keys and shapes of the reference's MultiScaleDiscriminator (recorded in the fixture; restated here): 80 entries"""
    out = {}
    for i in range(3):
        for l, p in enumerate(prefixes(i)):
            ci, co, k, _, g = LAYERS[l]
            out[p + 'bias'] = (co,)
            if i == 0:
                out[p + 'weight_orig'] = (co, ci // g, k)
                out[p + 'weight_u'] = (co,)
                out[p + 'weight_v'] = (ci // g * k,)
            else:
                out[p + 'weight_g'] = (co, 1, 1)
                out[p + 'weight_v'] = (co, ci // g, k)
    return out


def synth_state(shapes, seed, slope=SLOPE):
    """A seeded state in the style of hifigan_train_helpers.synth_state.  Weight-normed layers: weight_v ~ N(0, 1), weight_g about
    sqrt(2 / (1 + slope^2)) (the variance a LeakyReLU loses) - activations stay O(1) at every depth.  The spectral-normed discriminator:
    weight_orig ~ N(0, 1 / fan_in), weight_u / weight_v three power iterations from a random unit start; its normalised weight has spectral norm 1 by
    construction, so its activations shrink with depth whatever the state and the biases (0.1 N(0, 1)) carry the upper layers."""
    gen = torch.Generator().manual_seed(seed)
    gain = (2.0 / (1.0 + slope * slope)) ** 0.5
    st = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith('bias'):
            st[k] = 0.1 * torch.randn(shp, generator=gen)
        elif k.endswith('weight_g'):
            st[k] = gain * (0.8 + 0.4 * torch.rand(shp, generator=gen))
        elif k.endswith('weight_orig'):
            st[k] = torch.randn(shp, generator=gen) / float(np.prod(shp[1:])) ** 0.5
        elif k.endswith('weight_u') or (k.endswith('weight_v') and len(shp) == 1):
            t = torch.randn(shp, generator=gen)
            st[k] = t / t.norm()
        else:
            st[k] = torch.randn(shp, generator=gen)
    for k in sorted(st):                                        # a trained checkpoint's buffers: three power iterations from the random start
        if k.endswith('weight_orig'):
            p, W = k[:-len('weight_orig')], st[k].flatten(1)
            u = st[p + 'weight_u']
            for _ in range(3):
                v = W.t() @ u
                v = v / v.norm()
                u = W @ v
                u = u / u.norm()
            st[p + 'weight_u'], st[p + 'weight_v'] = u, v
    return st


def synth_plain(seed, slope=SLOPE):
    """plain float32 weights and biases of one DiscriminatorS with O(1) activations: rows of norm about the gain"""
    gen = torch.Generator().manual_seed(seed)
    gain = (2.0 / (1.0 + slope * slope)) ** 0.5
    ws, bs = [], []
    for ci, co, k, _, g in LAYERS:
        w = torch.randn(co, ci // g, k, generator=gen)
        ws.append(gain * (0.8 + 0.4 * torch.rand(co, 1, 1, generator=gen)) * w / w.flatten(1).norm(dim=1).reshape(-1, 1, 1))
        bs.append(0.1 * torch.randn(co, generator=gen))
    return ws, bs


# ---- the module, functionally (float64, with bounds) ------------------------------------------------------------------------------------------------
def disc_weights(state, i, power_iteration, e_state=None):
    """effective weights of discriminator i from a float64 state -> dict(ws, e_ws, bs, sp): sp the spectral64 results (discriminator 0), whose
    u / v are the buffers AFTER the call; e_state: bounds of the buffers handed in ({key: bound}, absent: exact)"""
    ws, e_ws, bs, sps = [], [], [], []
    e_state = e_state or {}
    for p in prefixes(i):
        bs.append(state[p + 'bias'])
        if i == 0:
            sp = spectral64(state[p + 'weight_orig'], state[p + 'weight_u'], state[p + 'weight_v'], power_iteration,
                            e_state.get(p + 'weight_u'), e_state.get(p + 'weight_v'))
            ws.append(sp['w']); e_ws.append(sp['e_w']); sps.append(sp)
        else:
            w, e = weight_norm_bound(state[p + 'weight_g'], state[p + 'weight_v'])
            ws.append(w); e_ws.append(e); sps.append(None)
    return dict(ws=ws, e_ws=e_ws, bs=bs, sp=sps)


def msd_forward64(state, y, y_hat, training):
    """MultiScaleDiscriminator.forward in float64 with bounds.  In training mode discriminator 0's buffers move once per d(.) call: d(y) uses
    the weights after one power iteration, d(y_hat) after two.  -> dict(r, g: per discriminator forward64 results + 'x', 'e_x', 'w' (disc_weights);
    state: the float64 state after the call)"""
    st = {k: d64(v) for k, v in state.items()}
    xs = {'r': (d64(y), None), 'g': (d64(y_hat), None)}
    out = {'r': [], 'g': []}
    est = {}
    for i in range(3):
        if i != 0:
            xs = {s: pool_bound(*xs[s]) for s in xs}
        for s in ('r', 'g'):
            wt = disc_weights(st, i, training, est)
            if i == 0 and training:
                for p, sp in zip(prefixes(0), wt['sp']):
                    st[p + 'weight_u'], st[p + 'weight_v'] = sp['u'], sp['v']
                    est[p + 'weight_u'], est[p + 'weight_v'] = sp['e_u'], sp['e_v']
            f = forward64(xs[s][0], wt['ws'], wt['bs'], e_ws=wt['e_ws'], e_x=xs[s][1])
            f.update(x=xs[s][0], e_x=xs[s][1], w=wt)
            out[s].append(f)
    out['state'], out['e_state'] = st, est
    return out


def msd_loss_bounds(fw):
    """bounds of msd_losses64's four values for a float32 evaluation of the maps with float64 sums: the maps' bounds through the means"""
    fl = 2 * sum(float((r['e_fmap'][l] + g['e_fmap'][l]).mean()) for r, g in zip(fw['r'], fw['g']) for l in range(N))
    def ls(f, t):
        p, e = f['fmap'][N - 1], f['e_fmap'][N - 1]
        return float((2 * (p - t).abs() * e + e * e).mean()) / 3
    vals = msd_losses64(fw)
    raw = (fl, sum(ls(f, 1.0) for f in fw['g']), sum(ls(f, 1.0) for f in fw['r']), sum(ls(f, 0.0) for f in fw['g']))
    return tuple(b + 64 * U * abs(float(v)) for b, v in zip(raw, vals))


def msd_losses64(fw):
    """(feature_loss, generator_loss, r_loss, g_loss) of hifigan.py:328-365 from msd_forward64's result, float64"""
    fl, _ = feature_loss64([f['fmap'] for f in fw['r']], [f['fmap'] for f in fw['g']])
    gen = sum(lsgan64(f['fmap'][N - 1], 1.0) for f in fw['g']) / 3
    rl = sum(lsgan64(f['fmap'][N - 1], 1.0) for f in fw['r']) / 3
    gl = sum(lsgan64(f['fmap'][N - 1], 0.0) for f in fw['g']) / 3
    return fl, gen, rl, gl


def msd_backward64(fw, state, T):
    """Gradients of L = feature_loss + generator_loss + r_loss + g_loss with bounds -> dict(grads {key: (value, bound)}, dy_hat (value, bound))"""
    st = {k: d64(v) for k, v in state.items()}
    grads, dyh, e_dyh = {}, None, None
    Ts = [T, T // 2, T // 2 // 2]
    for i in range(3):
        per_side = {}
        for s in ('r', 'g'):
            f = fw[s][i]
            o = fw['g' if s == 'r' else 'r'][i]
            cts, e_cts = [], []
            for l in range(N):
                r_, g_ = (f, o) if s == 'r' else (o, f)
                ct, e = l1_cotangents(r_['fmap'][l], g_['fmap'][l], r_['e_fmap'][l], g_['e_fmap'][l])
                cts.append(ct if s == 'r' else -ct); e_cts.append(e)
            p = f['fmap'][N - 1]
            if s == 'r':
                go, e_go = lsgan_ct(p, 1.0, 1.0 / 3, f['e_fmap'][N - 1])
            else:
                g1, e1 = lsgan_ct(p, 1.0, 1.0 / 3, f['e_fmap'][N - 1])
                g0, e0 = lsgan_ct(p, 0.0, 1.0 / 3, f['e_fmap'][N - 1])
                go, e_go = g1 + g0, e1 + e0 + U * (g1 + g0).abs()
            per_side[s] = backward64(go.reshape(p.shape[0], -1), cts, f['x'], f['w']['ws'], f['fmap'], e_acts=f['e_fmap'], e_ws=f['w']['e_ws'],
                                     e_g_fmap=e_cts, e_g_out=e_go.reshape(p.shape[0], -1))
        for l, p in enumerate(prefixes(i)):
            for s in ('r', 'g'):
                wt, bw = fw[s][i]['w'], per_side[s]
                (dw, e_dw), (db, e_db) = bw['dw'][l], bw['db'][l]
                if i == 0:
                    part = {p + 'weight_orig': spectral_grad64(st[p + 'weight_orig'], wt['sp'][l], dw, e_dw), p + 'bias': (db, e_db)}
                else:
                    (gg, e_gg), (gv, e_gv) = weight_norm_grads64(st[p + 'weight_g'], st[p + 'weight_v'], dw, e_dw)
                    part = {p + 'weight_g': (gg, e_gg), p + 'weight_v': (gv, e_gv), p + 'bias': (db, e_db)}
                for k, (v, e) in part.items():
                    if k in grads:
                        v0, e0 = grads[k]
                        grads[k] = (v0 + v, e0 + e + U * (v0 + v).abs())
                    else:
                        grads[k] = (v, e)
        d, e = per_side['g']['dx']
        for j in range(i, 0, -1):
            d, e = pool_backward_bound(d, e, Ts[j - 1])
        dyh, e_dyh = (d, e) if dyh is None else (dyh + d, e_dyh + e + U * (dyh + d).abs())
    return dict(grads=grads, dy_hat=(dyh, e_dyh))


# ---- the module as torch modules (the twin) -------------------------------------------------------------------------------------------------------
class TwinS(nn.Module):
    """hifigan.py:253-286 restated: torch Conv1d under torch's own norms"""

    def __init__(self, use_spectral_norm=False):
        super().__init__()
        from torch.nn.utils import spectral_norm, weight_norm
        norm_f = spectral_norm if use_spectral_norm else weight_norm
        mods = [norm_f(nn.Conv1d(ci, co, k, s, padding=(k - 1) // 2, groups=g)) for ci, co, k, s, g in LAYERS]
        self.convs = nn.ModuleList(mods[:-1])
        self.conv_post = mods[-1]

    def forward(self, x, mel=None):
        fmap = []
        for m in self.convs:
            x = F.leaky_relu(m(x), SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class TwinMSD(nn.Module):
    """hifigan.py:289-325 restated"""

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([TwinS(True), TwinS(), TwinS()])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=1), nn.AvgPool1d(4, 2, padding=1)])

    def forward(self, y, y_hat, mel=None):
        rs, gs, frs, fgs = [], [], [], []
        for i, d in enumerate(self.discriminators):
            if i != 0:
                y, y_hat = self.meanpools[i - 1](y), self.meanpools[i - 1](y_hat)
            r, fr = d(y)
            g, fg = d(y_hat)
            rs.append(r); gs.append(g); frs.append(fr); fgs.append(fg)
        return rs, gs, frs, fgs


def twin_losses(out):
    """the four losses from a module's four lists, with torch expressions (hifigan.py:328-365)"""
    rs, gs, frs, fgs = out
    fl = 0
    for dr, dg in zip(frs, fgs):
        for rl, gl in zip(dr, dg):
            fl = fl + torch.mean(torch.abs(rl - gl))
    gen = sum(torch.mean((1 - g) ** 2) for g in gs) / len(gs)
    rl_ = sum(torch.mean((1 - r) ** 2) for r in rs) / len(rs)
    gl_ = sum(torch.mean(g ** 2) for g in gs) / len(rs)
    return fl * 2, gen, rl_, gl_


# ---- fixture ---------------------------------------------------------------------------------------------------------------------------------------
def sample_index(numel, seed, n=FIXTURE_SAMPLES):
    """the fixed subsample of a tensor: every element when it has at most n, else n seeded distinct flat indices in ascending order"""
    if numel <= n:
        return np.arange(numel)
    return np.sort(np.random.RandomState(seed).permutation(numel)[:n])


def fixture():
    """tests/golden/hifigan_disc_ref.npz (tools/make_golden_hifigan_disc.py) -> dict of arrays; 'meta' is the decoded meta_json"""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files if k != 'meta_json'}
    out['meta'] = json.loads(str(z['meta_json']))
    return out


def fixture_inputs():
    """(state, y, y_hat) of the fixture's recipe: the seeded state rounded to float16 values (held in float32), seeded waveforms"""
    state = {k: v.half().float() for k, v in synth_state(module_shapes(), FIXTURE_SEED).items()}
    for k in state:                                             # the unit vectors stay unit vectors to float32
        if k.endswith('weight_u') or (k.endswith('weight_v') and state[k].dim() == 1):
            state[k] = state[k] / state[k].norm()
    gen = torch.Generator().manual_seed(FIXTURE_SEED + 1)
    y = 0.5 * torch.randn(FIXTURE_B, 1, FIXTURE_T, generator=gen)
    y_hat = y + 0.3 * torch.randn(FIXTURE_B, 1, FIXTURE_T, generator=gen)
    return state, y, y_hat


# ---- what the GPU tests of the period and the scale discriminator share (tests/test_gpu_hifigan_mpd.py, tests/test_gpu_hifigan_msd.py) ---------------
DEV = 'cuda'
NAN = float('nan')
GUARD = 64
CLOSE = 1e-4                            # the module-level figure of tests/test_hifigan_mpd_host.py and tests/test_hifigan_disc_host.py


def rnd(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def within(name, got, want, bound):
    err = (d64(got).reshape(want.shape) - want).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool(ok.all()), f'{name}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst error / bound {ratio:.3g}, max error {float(err.max()):.3g}'
    return ratio


def close(name, got, want, scale=None, tol=CLOSE):
    scale = want if scale is None else scale
    got = d64(got).reshape(want.shape)
    err, big = float((got - want).abs().max()), float(scale.abs().max())
    print(f'{name}: max error {err:.3e}, largest value {big:.3e}')
    assert err <= tol * big, f'{name}: max error {err:.3e} against the largest value {big:.3e}'


class Guarded:
    """device buffers between NaN guards (16-byte aligned: the guards are 64 floats)"""

    def __init__(self):
        self.all = []

    def new(self, *shape, src=None):
        n = 1
        for s in shape:
            n *= s
        raw = torch.full((n + 2 * GUARD,), NAN, device=DEV)
        v = raw[GUARD:GUARD + n].view(*shape)
        if src is not None:
            v.copy_(src.reshape(shape))
        self.all.append((raw, n))
        return v

    def check(self):
        for raw, n in self.all:
            assert bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[GUARD + n:]).all()), 'a guard was written'


class Ops:
    """the C ABI on the current stream; the test files add their own packing"""

    def __init__(self):
        from diffsinger_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.s = torch.cuda.current_stream().cuda_stream

    def call(self, name, *args):
        self.L.check(getattr(self.lib, name)(*args, self.s), name)

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()
