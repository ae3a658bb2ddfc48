"""HiFi-GAN discriminators on the HIP operators of include/dsv.h, sections "HiFi-GAN scale discriminator" (kernels: csrc/hifigan_disc.hpp),
"HiFi-GAN scale discriminator stack" (csrc/hifigan_msd.hpp) and "HiFi-GAN period discriminator" (csrc/hifigan_mpd.hpp).

    avg_pool_op                                AvgPool1d(4, 2, padding=1) of MultiScaleDiscriminator (modules/hifigan/hifigan.py:304-307), forward
                                               and backward
    generator_loss, discriminator_loss         pwg_disc's (hifigan.py:337-347, :359-365); cond_discriminator_loss hifigan.py:350-356
    disc_p_op                                  DiscriminatorP (hifigan.py:181-227) on plain weights, forward and backward through ONE autograd node
    feature_loss                               hifigan.py:328-334
    DiscriminatorP, MultiPeriodDiscriminator   hifigan.py:181-250: the reference's constructor signatures and state-dict keys
    disc_s_op                                  DiscriminatorS (hifigan.py:253-286) on plain weights - the grouped, strided Conv1d stack - forward and
                                               backward through ONE autograd node
    DiscriminatorS, MultiScaleDiscriminator    hifigan.py:253-325: the reference's constructor signatures and state-dict keys; spectral norm (with its
                                               power iteration in train()) and weight norm are torch expressions
    hifigan_adversarial_losses, hifigan_discriminator_losses       the generator's adversarial + feature-matching terms, the discriminator's pair

There is no CPU path.  Nothing here synchronises or reads a device value on the host, every launch goes to the current stream and the library
allocates nothing; recording these operators - the period discriminator's and the scale discriminator's alike - into a captured graph is UNVERIFIED
and UNSUPPORTED (no test or tool does it), and the capture fault of an earlier, unpublished version of the scale discriminator's kernels (DESIGN.md
section 6 "HiFi-GAN scale discriminator") is still unexplained: whoever records these operators into a graph has to explain it first.

The period discriminator's activations are the reference's tensors, dense [B][C][H][p]: the feature maps disc_p_op returns are views of the buffers
its kernels wrote, and the module runs d(y) and d(y_hat) as ONE batch of 2 B - every layer's weights stream once per pass - and hands out the two
halves of each buffer as outputs of the same node.  feature_loss writes the two cotangents of a pair into the halves of one buffer, which the node's
backward recognises (adjacent addresses) and reads in place: no feature map and no feature-map cotangent is copied on the module's path.
g * v / ||v|| and its gradient stay torch expressions.

Kernel launches through the library are counted by pwg_disc's counter (`launch_count()` is that function): avg_pool_op is one launch forward
and one backward; lsgan_loss_op 2 forward, 1 backward.  disc_p_op forward is 15: fold 1, first layer 1, per dense layer 3 (dsv_pack_weight's
kernel and slack fill, the convolution), conv_post 1.  Its backward is 37 + s + 2 x: conv_post 3 (parameter gradients, their reduction, data
gradient), per dense layer 1 weight gradient + 1 bias gradient (+ 1 reduction where dsv_hgp_wgrad_splits > 1: s counts those layers), its
data gradient 2 r + 1 (r = stride: one pack per input phase; 7, 7, 7, 3), the first layer 2, and x = 1 when the input requires a gradient: 2
more (first layer's data gradient, the fold's adjoint); a layer without a bias is one less.  feature_loss over n pairs is n + 1 forward, n backward.

The scale discriminator's activations are dense [B][C][L] and the same rules hold: the maps disc_s_op returns are views of its buffers, the module
runs d(y) and d(y_hat) as one batch of 2 B (pooled as one batch, too) wherever the weights are the same for both - the weight-normed
discriminators always, the spectral-normed one in eval(); in train() its buffers move between the two calls, so it runs twice, y first.
disc_s_op forward is 15 launches: first layer 1, per grouped layer 2 (dsv_hgs_pack, dsv_hgs_gconv), the dense layer 3 (dsv_pack_weight's two, dsv_hgp_conv
at period 1), conv_post 1 (dsv_hgp_post).  Its backward is 30 + s + x: conv_post 3, the dense layer 5 (weight gradient, bias gradient, the pack's
two, data gradient), per grouped layer 4 (weight gradient, bias gradient, dsv_hgs_pack of the phase matrices, data gradient; + 1 reduction where
dsv_hgs_wgrad_splits > 1: s counts those layers), the first layer 2 and x = 1 when the input requires a gradient; a layer without a bias is one less.

DiscPFunction and DiscSFunction are the two autograd nodes; their forwards differ (the fold, the per-layer kernels) and so do the first and the
grouped layers of their backwards.  Everything else exists once and serves both: _hand_out / _pair_results (the outputs, or their halves under
pair=True, and the inverse), _gather_cots (the cotangents' addresses; _join alone owns the adjacent-halves rule), _grad_buffers, _post_backward,
_dense_backward (the scale discriminator's layer 6 is the period discriminator's layer 4 at period 1, stride 1; the first layers keep a
kernel set each), _check_params (driven by a list of weight shapes), _check_pair and the modules' base classes _Disc (all four) and
_SingleDisc (the two single discriminators' _params).  _grad_buffers allocates every gradient before the first launch, not layer by layer."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from .pwg import _WN
from .pwg_disc import _call, _check_x as _check_pwg_x, discriminator_loss, generator_loss, launch_count, lsgan_loss_op
from .vocoder import padded_samples

__all__ = ['avg_pool_op', 'generator_loss', 'discriminator_loss', 'cond_discriminator_loss', 'launch_count', 'disc_p_op', 'feature_loss',
           'DiscriminatorP', 'MultiPeriodDiscriminator', 'hifigan_adversarial_losses', 'hifigan_discriminator_losses', 'period_heights',
           'disc_s_op', 'DiscriminatorS', 'MultiScaleDiscriminator', 'scale_lengths']


def _check_x(x, who, min_t=1):
    if isinstance(x, torch.Tensor) and x.dim() == 3 and 1 <= x.shape[2] < min_t:
        raise ValueError(f'{who}: x must have T >= {min_t} samples, got {tuple(x.shape)}')
    _check_pwg_x(x, who)


class AvgPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, _, T = x.shape
        out = torch.empty(B, padded_samples(T // 2), device=x.device, dtype=torch.float32)
        _call('dsv_hgd_avgpool', 1, x.device, x.data_ptr(), out.data_ptr(), B, T, T)
        ctx.meta = (B, T)
        return out[:, None, :T // 2]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, T = ctx.meta
        g = g.to(torch.float32).contiguous()
        dx = torch.empty(B, padded_samples(T), device=g.device, dtype=torch.float32)
        _call('dsv_hgd_avgpool_backward', 1, g.device, g.data_ptr(), dx.data_ptr(), B, T, T // 2)
        return dx[:, None, :T]


def avg_pool_op(x):
    """AvgPool1d(4, 2, padding=1) (count_include_pad: the divisor is always 4) of x float32 [B][1][T], T >= 2 -> [B][1][T // 2]"""
    _check_x(x, 'avg_pool_op', 2)
    return AvgPoolFunction.apply(x.contiguous())


def cond_discriminator_loss(outputs):
    """modules/hifigan/hifigan.py:350-356: mean over the discriminators of mean(D(G(z))^2)."""
    loss = 0
    for dg in outputs:
        loss = loss + lsgan_loss_op(dg, 0.0)
    return loss / len(outputs)


# ---- the period discriminator -----------------------------------------------------------------------------------------------------------------
_CH = (1, 32, 128, 512, 1024, 1024)                              # channels in front of conv l (hifigan.py:193-199); conv_post 1024 -> 1
_STRIDES = (3, 3, 3, 3, 1)
_NCONV = 5
_K, _KPOST = 5, 3
_PERIODS = (2, 3, 5, 7, 11)
LRELU_SLOPE = 0.1


def period_heights(T: int, period: int):
    """[H0 .. H4, H4]: the input height of conv l (l = 0..4) and of conv_post, for T samples at this period; ValueError where the reference's
    reflect pad refuses T (the pad period - T mod period is not shorter than T)"""
    T, period = int(T), int(period)
    if period < 1 or T < 1:
        raise ValueError(f'period_heights: T={T} and period={period} must be >= 1')
    n_pad = (period - T % period) % period
    if n_pad >= T:
        raise ValueError(f'DiscriminatorP: T={T} at period {period} needs a reflect pad of {n_pad} >= T samples')
    hs = [(T + n_pad) // period]
    for s in _STRIDES:
        hs.append((hs[-1] - 1) // s + 1)
    return hs


def _phase_taps(lib, stride, r):
    m = lib.dsv_hgp_dgrad_phase_taps(stride, r)
    return [k for k in range(_K) if m >> k & 1]


def _f32c(t):
    return None if t is None else t.to(torch.float32).contiguous()


def _join(cr, cg, shape, dev):
    """the cotangents of the two halves of a buffer of `shape` as (address, what keeps it alive): in place where they are the halves of one
    buffer (feature_loss's), else joined; (None, None) where neither arrives"""
    if cr is None and cg is None:
        return None, None
    Bh = shape[0] // 2
    cr, cg = _f32c(cr), _f32c(cg)
    if cr is not None and cg is not None and cg.data_ptr() == cr.data_ptr() + 4 * cr.numel():
        return cr.data_ptr(), (cr, cg)
    t = torch.zeros(shape, device=dev, dtype=torch.float32)
    if cr is not None:
        t[:Bh] = cr.reshape(t[:Bh].shape)
    if cg is not None:
        t[Bh:] = cg.reshape(t[Bh:].shape)
    return t.data_ptr(), t


# ---- what the two autograd nodes share ----------------------------------------------------------------------------------------------------------
def _hand_out(out, maps, pair):
    """what a node's forward returns: (out,) + maps, or with pair=True every buffer as its two halves, (out_r, out_g, the maps' first halves, the
    second halves)"""
    if not pair:
        return (out,) + tuple(maps)
    Bh = out.shape[0] // 2
    return (out[:Bh], out[Bh:]) + tuple(m[:Bh] for m in maps) + tuple(m[Bh:] for m in maps)


def _pair_results(res, n):
    """_hand_out's inverse for pair=True and n maps: ((out_r, fmap_r), (out_g, fmap_g)), every tensor a half of the node's buffers"""
    return (res[0], list(res[2:2 + n])), (res[1], list(res[2 + n:]))


def _gather_cots(cots, pair, shapes, dev):
    """the cotangents a node's backward receives, for _hand_out's outputs over maps of `shapes` (the last one conv_post's, whose flattening is out)
    -> (gp1, gp2, cot, keep): the addresses of the one or two cotangents of conv_post's output (gp2 None where one arrives; a zero buffer where
    none does), the per-map addresses (None where absent) and the tensors that keep all of them alive"""
    n = len(shapes)
    out_shape = (shapes[-1][0], math.prod(shapes[-1][1:]))
    keep, cot = [], []
    if pair:
        g_out, k = _join(cots[0], cots[1], out_shape, dev)
        keep.append(k)
        for l in range(n):
            a, k = _join(cots[2 + l], cots[2 + n + l], shapes[l], dev)
            cot.append(a); keep.append(k)
    else:
        t = _f32c(cots[0])
        g_out = None if t is None else t.data_ptr()
        keep.append(t)
        for l in range(n):
            t = _f32c(cots[1 + l])
            cot.append(None if t is None else t.data_ptr()); keep.append(t)
    gp1, gp2 = (g_out, cot[-1]) if g_out is not None else (cot[-1], None)
    if gp1 is None:                                             # nothing arrives on the output: its cotangent is zero
        z = torch.zeros(out_shape, device=dev, dtype=torch.float32)
        keep.append(z)
        gp1 = z.data_ptr()
    return gp1, gp2, cot, keep


def _grad_buffers(wshapes, has_b, dev):
    """(dws, dbs): one weight gradient per shape, one bias gradient (None where the layer has no bias)"""
    return ([torch.empty(s, device=dev, dtype=torch.float32) for s in wshapes],
            [torch.empty(s[0], device=dev, dtype=torch.float32) if hb else None for s, hb in zip(wshapes, has_b)])


def _hp(a):
    """(H, p) of an activation [B][C][H][p], or [B][C][L] of the scale discriminator: (L, 1)"""
    return a.shape[2], (a.shape[3] if a.dim() == 4 else 1)


def _post_backward(gp1, gp2, a, w, cot, ws_e, dw, db, slope):
    """conv_post's backward over its input a: parameter gradients into dw / db through the workspace ws_e -> the gradient with respect to the
    pre-activation behind a, which includes the cotangent `cot` of a"""
    H, p = _hp(a)
    G = torch.empty(a.shape, device=a.device, dtype=torch.float32)
    _call('dsv_hgp_post_backward', 3, a.device, gp1, gp2, a.data_ptr(), w.data_ptr(), cot, ws_e.data_ptr(), dw.data_ptr(), _lib.ptr(db), G.data_ptr(),
          a.shape[0], a.shape[1], H, p, slope)
    return G


def _dense_backward(lib, G, a, w, cot, dw, db, S, slope):
    """backward of a dense K = 5 layer w [Co][Ci][5] of stride S over its input a, G the gradient with respect to its pre-activation:
    dsv_hgp_conv_wgrad into dw / db, dsv_pack_weight per input phase, dsv_hgp_conv_dgrad -> the gradient with respect to the pre-activation
    behind a, which includes the cotangent `cot` of a.  The scale discriminator's layer 6 is the period discriminator's layer 4 at period 1."""
    dev, B = a.device, a.shape[0]
    (H, p), (co, ci) = _hp(a), w.shape[:2]
    nws = lib.dsv_hgp_wgrad_workspace_floats(B, ci, co, G.shape[2], p)
    ws_w = torch.empty(nws, device=dev, dtype=torch.float32) if nws else None
    _call('dsv_hgp_conv_wgrad', 1 + (1 if nws else 0) + (0 if db is None else 1), dev, G.data_ptr(), a.data_ptr(), _lib.ptr(ws_w), dw.data_ptr(),
          _lib.ptr(db), B, ci, co, H, p, S)
    packed = torch.empty(lib.dsv_hgp_dgrad_packed_offset(ci, co, S, S), device=dev, dtype=torch.float32)
    for r in range(S):
        ks = _phase_taps(lib, S, r)
        m = (w if len(ks) == _K else w[:, :, ks]).permute(1, 0, 2).contiguous()     # [ci][co][taps of the phase]; stride 1: the one phase holds all five
        _call('dsv_pack_weight', 2, dev, m.data_ptr(), ci, co, len(ks), packed.data_ptr() + 4 * lib.dsv_hgp_dgrad_packed_offset(ci, co, S, r))
    Gn = torch.empty(a.shape, device=dev, dtype=torch.float32)
    _call('dsv_hgp_conv_dgrad', 1, dev, G.data_ptr(), packed.data_ptr(), cot, a.data_ptr(), Gn.data_ptr(), B, ci, co, H, p, S, slope)
    return Gn


class DiscPFunction(torch.autograd.Function):
    """x [B][1][T], six weights [Co][Ci][K][1], six biases (None where absent) -> (out [B][H p], a_0 .. a_4, a_5 = conv_post's output [B][1][H][p]):
    views of the node's buffers.  pair=True: B = 2 Bh and every output is handed out as its two halves, (out_r, out_g, the six maps' first halves,
    the six second halves)."""

    @staticmethod
    def forward(ctx, x, period, slope, pair, *params):
        lib = _lib.load()
        ws, bs = params[:_NCONV + 1], params[_NCONV + 1:]
        dev = x.device
        B, _, T = x.shape
        p = period
        hs = period_heights(T, p)
        xf = torch.empty(B, hs[0] * p, device=dev, dtype=torch.float32)
        _call('dsv_hgp_fold', 1, dev, x.data_ptr(), xf.data_ptr(), B, T, T, p)
        wd = [w.detach().reshape(w.shape[0], w.shape[1], w.shape[2]).contiguous() for w in ws]
        b = [None if t is None else t.detach().contiguous() for t in bs]
        acts = [torch.empty(B, _CH[l + 1], hs[l + 1], p, device=dev, dtype=torch.float32) for l in range(_NCONV)]
        _call('dsv_hgp_first', 1, dev, xf.data_ptr(), wd[0].data_ptr(), _lib.ptr(b[0]), acts[0].data_ptr(), B, _CH[1], hs[0], p, _STRIDES[0], slope)
        for l in range(1, _NCONV):
            ci, co = _CH[l], _CH[l + 1]
            packed = torch.empty(lib.dsv_packed_floats(co, ci, _K), device=dev, dtype=torch.float32)
            _call('dsv_pack_weight', 2, dev, wd[l].data_ptr(), co, ci, _K, packed.data_ptr())
            _call('dsv_hgp_conv', 1, dev, acts[l - 1].data_ptr(), packed.data_ptr(), _lib.ptr(b[l]), acts[l].data_ptr(), B, ci, co, hs[l], p, _STRIDES[l],
                  slope)
        post = torch.empty(B, 1, hs[5], p, device=dev, dtype=torch.float32)
        _call('dsv_hgp_post', 1, dev, acts[4].data_ptr(), wd[5].data_ptr(), _lib.ptr(b[5]), post.data_ptr(), B, _CH[5], hs[5], p)
        ctx.save_for_backward(xf, *wd, *acts)
        ctx.meta = (B, T, p, float(slope), bool(pair), hs, [t is not None for t in bs])
        return _hand_out(post.view(B, hs[5] * p), acts + [post], pair)

    @staticmethod
    @once_differentiable
    def backward(ctx, *cots):
        lib = _lib.load()
        xf, *rest = ctx.saved_tensors
        wd, acts = rest[:_NCONV + 1], rest[_NCONV + 1:]
        B, T, p, slope, pair, hs, has_b = ctx.meta
        dev = xf.device
        gp1, gp2, cot, keep = _gather_cots(cots, pair, [a.shape for a in acts] + [(B, 1, hs[5], p)], dev)    # keep: tensors whose addresses are in flight
        dws, dbs = _grad_buffers([tuple(w.shape) + (1,) for w in wd], has_b, dev)
        ws_e = torch.empty(max(lib.dsv_hgp_edge_workspace_floats(B, hs[5], p, _CH[5], _KPOST), lib.dsv_hgp_edge_workspace_floats(B, hs[1], p, _CH[1], _K)),
                           device=dev, dtype=torch.float32)
        G = _post_backward(gp1, gp2, acts[4], wd[5], cot[4], ws_e, dws[5], dbs[5], slope)
        for l in range(_NCONV - 1, 0, -1):
            G = _dense_backward(lib, G, acts[l - 1], wd[l], cot[l - 1], dws[l], dbs[l], _STRIDES[l], slope)
        need_dx = ctx.needs_input_grad[0]
        dxf = torch.empty(B, hs[0] * p, device=dev, dtype=torch.float32) if need_dx else None
        _call('dsv_hgp_first_backward', 3 if need_dx else 2, dev, G.data_ptr(), xf.data_ptr(), wd[0].data_ptr(), ws_e.data_ptr(), dws[0].data_ptr(),
              _lib.ptr(dbs[0]), _lib.ptr(dxf), B, _CH[1], hs[0], p, _STRIDES[0])
        gx = None
        if need_dx:
            dx = torch.empty(B, T, device=dev, dtype=torch.float32)
            _call('dsv_hgp_fold_backward', 1, dev, dxf.data_ptr(), dx.data_ptr(), B, T, p)
            gx = dx[:, None, :]
        del keep
        return (gx, None, None, None) + tuple(dws) + tuple(dbs)


def _check_px(x, period, who):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f'{who}: x must be a tensor')
    if x.dim() != 3 or x.shape[1] != 1 or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f'{who}: x must be [B][1][T] with B >= 1 and T >= 1, got {tuple(x.shape)}')
    if not isinstance(period, int) or not 1 <= period <= 64:
        raise ValueError(f'{who}: period={period!r} must be an integer in [1, 64]')
    hs = period_heights(x.shape[2], period)
    _check_pwg_x(x, who)
    if x.shape[0] * period > 65535:
        raise ValueError(f'{who}: B * period = {x.shape[0] * period} exceeds 65535')
    return hs


_P_SHAPES = [(_CH[l + 1], _CH[l], _K, 1) for l in range(_NCONV)] + [(1, _CH[_NCONV], _KPOST, 1)]


def _check_params(x, weights, biases, slope, who, shapes=_P_SHAPES, n='six'):
    """plain weights of `shapes` ([Co] first) and biases [Co] or None, float32 on x's device; n: their number in words, for the message"""
    if len(weights) != len(shapes) or len(biases) != len(shapes):
        raise ValueError(f'{who}: {n} weights and {n} biases (None where absent), got {len(weights)} and {len(biases)}')
    if not 0.0 < float(slope) < 1.0:
        raise ValueError(f'{who}: slope={slope} must be in (0, 1)')

    def bad(t, want):
        return not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != torch.float32 or t.device != x.device

    def what(t):
        return f'{t.dtype} {tuple(t.shape)} on {t.device}' if isinstance(t, torch.Tensor) else type(t).__name__

    for i, (w, bi, want) in enumerate(zip(weights, biases, shapes)):
        if bad(w, want):
            raise ValueError(f'{who}: weights[{i}] must be float32 {want} on {x.device}, got {what(w)}')
        if bi is not None and bad(bi, want[:1]):
            raise ValueError(f'{who}: biases[{i}] must be float32 ({want[0]},) on {x.device}, got {what(bi)}')


def disc_p_op(x, period: int, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]], slope: float = LRELU_SLOPE):
    """DiscriminatorP.forward on plain weights: weights[l] [Co][Ci][5][1] for the five convs (1 -> 32 -> 128 -> 512 -> 1024 -> 1024, stride 3, 3, 3, 3,
    1), weights[5] [1][1024][3][1]; biases[l] [Co] or None; x float32 [B][1][T] on the device -> (out [B][H p], fmap): the six feature maps
    [B][C][H_l][p], views of the node's own buffers (fmap[5] and out are the same values).  Differentiable with respect to x, every weight and
    every bias; cotangents are accepted on out and on every map."""
    _check_px(x, period, 'disc_p_op')
    _check_params(x, weights, biases, slope, 'disc_p_op')
    res = DiscPFunction.apply(x.contiguous(), period, float(slope), False, *weights, *biases)
    return res[0], list(res[1:])


def _disc_p_pair(yy, period, weights, biases, slope):
    """disc_p_op over cat(y, y_hat): ((out_r, fmap_r), (out_g, fmap_g)), every tensor a half of the node's buffers"""
    return _pair_results(DiscPFunction.apply(yy, period, float(slope), True, *weights, *biases), _NCONV + 1)


class FeatureLossFunction(torch.autograd.Function):
    """n, r_0 .. r_{n-1}, g_0 .. g_{n-1} (float32, contiguous, pairwise equal shapes) -> 0-dim 2 sum_i mean|r_i - g_i|"""

    @staticmethod
    def forward(ctx, n, *ts):
        lib = _lib.load()
        dev = ts[0].device
        blocks = [lib.dsv_hgp_l1_blocks(t.numel()) for t in ts[:n]]
        ws = torch.empty(sum(blocks), device=dev, dtype=torch.float64)
        off = 0
        for i in range(n):
            _call('dsv_hgp_l1_partial', 1, dev, ts[i].data_ptr(), ts[n + i].data_ptr(), ws.data_ptr() + 8 * off, ts[i].numel())
            off += blocks[i]
        out = torch.empty(1, device=dev, dtype=torch.float32)
        _call('dsv_hgp_l1_final', 1, dev, ws.data_ptr(), off, out.data_ptr())
        ctx.save_for_backward(*ts)
        ctx.n = n
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ts, n = ctx.saved_tensors, ctx.n
        g = g.to(torch.float32).reshape(1).contiguous()
        dr, dg = [], []
        for i in range(n):
            buf = torch.empty((2,) + tuple(ts[i].shape), device=g.device, dtype=torch.float32)      # the two cotangents, adjacent: DiscPFunction reads them in place
            _call('dsv_hgp_l1_backward', 1, g.device, ts[i].data_ptr(), ts[n + i].data_ptr(), g.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(),
                  ts[i].numel())
            dr.append(buf[0]); dg.append(buf[1])
        return (None,) + tuple(dr) + tuple(dg)


def feature_loss(fmap_r, fmap_g):
    """modules/hifigan/hifigan.py:328-334: 2 * the sum over the discriminators and their maps of mean|r - g| -> 0-dim float32; float64 sums in a fixed
    order.  fmap_r, fmap_g: lists of lists of float32 device tensors of pairwise equal shapes (a discriminator's maps, or any tensors)."""
    rs = [t for d in fmap_r for t in d]
    gs = [t for d in fmap_g for t in d]
    if not rs or len(rs) != len(gs):
        raise ValueError(f'feature_loss: as many real as generated maps, at least one; got {len(rs)} and {len(gs)}')
    for i, (r, g) in enumerate(zip(rs, gs)):
        for t in (r, g):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.numel() < 1:
                what = f'{t.dtype} {tuple(t.shape)} on {t.device}' if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f'feature_loss: map {i} must be a non-empty float32 device tensor (there is no CPU path), got {what}')
        if r.shape != g.shape or r.device != g.device:
            raise ValueError(f'feature_loss: map {i}: {tuple(r.shape)} on {r.device} against {tuple(g.shape)} on {g.device}')
    return FeatureLossFunction.apply(len(rs), *[t.contiguous() for t in rs], *[t.contiguous() for t in gs])


class _Disc(nn.Module):
    """what the four discriminator modules share: members that are _WN holders (directly or in `discriminators`), no mel input"""

    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, _WN):
                m.remove_weight_norm()

    def _refuse_mel(self, mel):
        if mel is not None:
            raise NotImplementedError(f'{type(self).__name__} on HIP: use_cond (a mel input) is not supported')


class _SingleDisc(_Disc):
    """one discriminator: convs and conv_post hold its parameters"""

    @staticmethod
    def _weight(m):
        return torch._weight_norm(m.weight_v, m.weight_g, 0) if hasattr(m, 'weight_g') else m.weight

    def _params(self):
        mods = list(self.convs) + [self.conv_post]
        return [self._weight(m) for m in mods], [m.bias for m in mods]


def _check_pair(y, y_hat, who):
    """y_hat against a checked y: the second half of the batch of 2 B"""
    _check_pwg_x(y_hat, who)
    if y_hat.shape != y.shape or y_hat.device != y.device:
        raise ValueError(f'{who}: y {tuple(y.shape)} on {y.device} against y_hat {tuple(y_hat.shape)} on {y_hat.device}')


class DiscriminatorP(_SingleDisc):
    """modules/hifigan/hifigan.py:181-227.  forward(x [B,1,T], mel=None) -> (out [B, H p], fmap: six maps [B, C, H_l, p]), differentiable with respect
    to x and every parameter.  convs[l] / conv_post hold weight_g [Co,1,1,1], weight_v [Co,Ci,K,1], bias (or weight after remove_weight_norm())."""

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False, use_cond=False, c_in=1):
        super().__init__()
        bad = []
        if use_cond:
            bad.append('use_cond (the mel-conditioned input)')
        if c_in != 1:
            bad.append('c_in other than 1')
        if use_spectral_norm:
            bad.append('spectral norm')
        if kernel_size != _K or stride != 3:
            bad.append('kernel_size / stride other than 5 / 3')
        if bad:
            raise NotImplementedError('DiscriminatorP on HIP covers the shipped configuration only: ' + '; '.join(bad))
        if not isinstance(period, int) or not 1 <= period <= 64:
            raise ValueError(f'DiscriminatorP: period={period!r} must be an integer in [1, 64]')
        self.period, self.use_cond = period, False
        self.convs = nn.ModuleList([_WN((_CH[l + 1], _CH[l], _K, 1), True, True) for l in range(_NCONV)])
        self.conv_post = _WN((1, _CH[_NCONV], _KPOST, 1), True, True)

    def forward(self, x, mel=None):
        self._refuse_mel(mel)
        ws, bs = self._params()
        return disc_p_op(x, self.period, ws, bs, LRELU_SLOPE)


class MultiPeriodDiscriminator(_Disc):
    """modules/hifigan/hifigan.py:230-250: periods 2, 3, 5, 7, 11.  forward(y, y_hat, mel=None) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs).  d(y) and
    d(y_hat) run as one batch of 2 B per period (weight norm has no per-call state: the two calls of the reference use identical weights)."""

    def __init__(self, use_cond=False, c_in=1):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(p, use_cond=use_cond, c_in=c_in) for p in _PERIODS])

    def forward(self, y, y_hat, mel=None):
        self._refuse_mel(mel)
        for d in self.discriminators:
            _check_px(y, d.period, 'MultiPeriodDiscriminator')
        _check_pair(y, y_hat, 'MultiPeriodDiscriminator')
        yy = torch.cat([y, y_hat]).contiguous()
        rs, gs, frs, fgs = [], [], [], []
        for d in self.discriminators:
            ws, bs = d._params()
            _check_params(yy, ws, bs, LRELU_SLOPE, 'MultiPeriodDiscriminator')
            (r, fr), (g, fg) = _disc_p_pair(yy, d.period, ws, bs, LRELU_SLOPE)
            rs.append(r); gs.append(g); frs.append(fr); fgs.append(fg)
        return rs, gs, frs, fgs


# ---- the scale discriminator ------------------------------------------------------------------------------------------------------------------
# (Ci, Co, K, stride, groups), padding (K - 1) / 2: hifigan.py:263-271; conv_post 1024 -> 1
_S_LAYERS = ((1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (256, 512, 41, 4, 16), (512, 1024, 41, 4, 16), (1024, 1024, 41, 1, 16),
             (1024, 1024, 5, 1, 1), (1024, 1, 3, 1, 1))
_SN_LAYERS = len(_S_LAYERS)


def scale_lengths(T: int):
    """[L_0 .. L_7]: the output length of every layer of DiscriminatorS for T samples, (L - 1) // stride + 1"""
    T = int(T)
    if T < 1:
        raise ValueError(f'scale_lengths: T={T} must be >= 1')
    out = []
    for _, _, _, s, _ in _S_LAYERS:
        T = (T - 1) // s + 1
        out.append(T)
    return out


class DiscSFunction(torch.autograd.Function):
    """x [B][1][T] (rows ld >= T floats apart), eight weights [Co][Ci / g][K], eight biases (None where absent) -> (out [B][L_7], a_0 .. a_6, a_7 =
    conv_post's output [B][1][L_7]): views of the node's buffers.  pair=True: B = 2 Bh and every output is handed out as its two halves, (out_r,
    out_g, the eight maps' first halves, the eight second halves)."""

    @staticmethod
    def forward(ctx, x, slope, pair, *params):
        lib = _lib.load()
        n = _SN_LAYERS
        ws, bs = params[:n], params[n:]
        dev = x.device
        B, _, T = x.shape
        ld = x.stride(0) if B > 1 else T
        ls = scale_lengths(T)
        wd = [w.detach().contiguous() for w in ws]
        b = [None if t is None else t.detach().contiguous() for t in bs]
        acts = [torch.empty(B, _S_LAYERS[l][1], ls[l], device=dev, dtype=torch.float32) for l in range(n - 1)]
        _call('dsv_hgs_first', 1, dev, x.data_ptr(), wd[0].data_ptr(), _lib.ptr(b[0]), acts[0].data_ptr(), B, _S_LAYERS[0][1], T, ld, slope)
        for l in range(1, 6):
            ci, co, _, s, g = _S_LAYERS[l]
            packed = torch.empty(lib.dsv_hgs_packed_floats(ci, co, s, g, 0), device=dev, dtype=torch.float32)
            _call('dsv_hgs_pack', 1, dev, wd[l].data_ptr(), packed.data_ptr(), ci, co, s, g, 0)
            _call('dsv_hgs_gconv', 1, dev, acts[l - 1].data_ptr(), packed.data_ptr(), _lib.ptr(b[l]), acts[l].data_ptr(), B, ci, co, ls[l - 1], s, g, slope)
        ci, co, k = _S_LAYERS[6][:3]
        packed = torch.empty(lib.dsv_packed_floats(co, ci, k), device=dev, dtype=torch.float32)
        _call('dsv_pack_weight', 2, dev, wd[6].data_ptr(), co, ci, k, packed.data_ptr())
        _call('dsv_hgp_conv', 1, dev, acts[5].data_ptr(), packed.data_ptr(), _lib.ptr(b[6]), acts[6].data_ptr(), B, ci, co, ls[5], 1, 1, slope)
        post = torch.empty(B, 1, ls[7], device=dev, dtype=torch.float32)
        _call('dsv_hgp_post', 1, dev, acts[6].data_ptr(), wd[7].data_ptr(), _lib.ptr(b[7]), post.data_ptr(), B, _S_LAYERS[7][0], ls[7], 1)
        ctx.save_for_backward(x, *wd, *acts)
        ctx.meta = (B, T, ld, float(slope), bool(pair), ls, [t is not None for t in bs])
        return _hand_out(post.view(B, ls[7]), acts + [post], pair)

    @staticmethod
    @once_differentiable
    def backward(ctx, *cots):
        lib = _lib.load()
        n = _SN_LAYERS
        x, *rest = ctx.saved_tensors
        wd, acts = rest[:n], rest[n:]
        B, T, ld, slope, pair, ls, has_b = ctx.meta
        dev = x.device
        gp1, gp2, cot, keep = _gather_cots(cots, pair, [a.shape for a in acts] + [(B, 1, ls[7])], dev)       # keep: tensors whose addresses are in flight
        dws, dbs = _grad_buffers([w.shape for w in wd], has_b, dev)
        C = _S_LAYERS[7][0]
        ws_e = torch.empty(lib.dsv_hgp_edge_workspace_floats(B, ls[7], 1, C, _KPOST), device=dev, dtype=torch.float32)
        G = _post_backward(gp1, gp2, acts[6], wd[7], cot[6], ws_e, dws[7], dbs[7], slope)
        G = _dense_backward(lib, G, acts[5], wd[6], cot[5], dws[6], dbs[6], 1, slope)       # the period discriminator's fifth layer at period 1
        for l in range(5, 0, -1):
            ci, co, _, s, g = _S_LAYERS[l]
            nws = lib.dsv_hgs_wgrad_workspace_floats(B, ci, co, ls[l], s, g)
            ws_w = torch.empty(nws, device=dev, dtype=torch.float32) if nws else None
            _call('dsv_hgs_gconv_wgrad', 1 + (1 if nws else 0) + (1 if has_b[l] else 0), dev, G.data_ptr(), acts[l - 1].data_ptr(), _lib.ptr(ws_w),
                  dws[l].data_ptr(), _lib.ptr(dbs[l]), B, ci, co, ls[l - 1], s, g)
            packed = torch.empty(lib.dsv_hgs_packed_floats(ci, co, s, g, 1), device=dev, dtype=torch.float32)
            _call('dsv_hgs_pack', 1, dev, wd[l].data_ptr(), packed.data_ptr(), ci, co, s, g, 1)
            Gn = torch.empty(B, ci, ls[l - 1], device=dev, dtype=torch.float32)
            _call('dsv_hgs_gconv_dgrad', 1, dev, G.data_ptr(), packed.data_ptr(), cot[l - 1], acts[l - 1].data_ptr(), Gn.data_ptr(), B, ci, co, ls[l - 1], s, g,
                  slope)
            G = Gn
        C = _S_LAYERS[0][1]
        need_dx = ctx.needs_input_grad[0]
        ws_f = torch.empty(lib.dsv_hgs_first_workspace_floats(B, T, C), device=dev, dtype=torch.float32)
        dx = torch.empty(B, T, device=dev, dtype=torch.float32) if need_dx else None
        _call('dsv_hgs_first_backward', 3 if need_dx else 2, dev, G.data_ptr(), x.data_ptr(), wd[0].data_ptr(), ws_f.data_ptr(), dws[0].data_ptr(),
              _lib.ptr(dbs[0]), _lib.ptr(dx), B, C, T, ld)
        del keep
        return (None if dx is None else dx[:, None, :], None, None) + tuple(dws) + tuple(dbs)


def _check_sx(x, who, min_t=1):
    _check_x(x, who, min_t)
    if x.shape[2] > 1 << 30:
        raise ValueError(f'{who}: x has T={x.shape[2]} > 2^30 samples')


_S_SHAPES = [(co, ci // g, k) for ci, co, k, _, g in _S_LAYERS]


def _rows(x):
    """x [B][1][T] as the kernels take it: rows of unit stride, at least T floats apart (avg_pool_op's view is one), else a dense copy"""
    B, _, T = x.shape
    if x.stride(2) == 1 and (B == 1 or x.stride(0) >= T) and x.stride(0) <= 1 << 31:
        return x
    return x.contiguous()


def disc_s_op(x, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]], slope: float = LRELU_SLOPE):
    """DiscriminatorS.forward on plain weights: weights[l] [Co][Ci / groups][K] for the seven convs (1 -> 128 K 15; 128 -> 128, 128 -> 256, 256 -> 512,
    512 -> 1024, 1024 -> 1024 at K 41, stride 2, 2, 4, 4, 1, groups 4, 16, 16, 16, 16; 1024 -> 1024 K 5), weights[7] [1][1024][3]; biases[l] [Co] or
    None; x float32 [B][1][T] on the device -> (out [B][L_7], fmap): the eight feature maps [B][C][L_l], views of the node's own buffers (fmap[7]
    and out are the same values).  Differentiable with respect to x, every weight and every bias; cotangents are accepted on out and on every map."""
    _check_sx(x, 'disc_s_op')
    _check_params(x, weights, biases, slope, 'disc_s_op', _S_SHAPES, 'eight')
    res = DiscSFunction.apply(_rows(x), float(slope), False, *weights, *biases)
    return res[0], list(res[1:])


def _disc_s_pair(yy, weights, biases, slope):
    """disc_s_op over cat(y, y_hat): ((out_r, fmap_r), (out_g, fmap_g)), every tensor a half of the node's buffers"""
    return _pair_results(DiscSFunction.apply(_rows(yy), float(slope), True, *weights, *biases), _SN_LAYERS)


class _SN(nn.Module):
    """spectral_norm(Conv1d) parameter holder with torch.nn.utils.spectral_norm's state-dict keys - bias, weight_orig, buffers weight_u [Co] and
    weight_v [Ci / g K] - and its semantics: in train() every weight() call does one power iteration on the buffers under no_grad (v =
    normalize(W^T u), u = normalize(W v), in place), then sigma = u . (W v) with u and v constant and weight = W / sigma; in eval() no iteration."""

    def __init__(self, wshape, eps=1e-12):
        super().__init__()
        self.eps = eps
        self.bias = nn.Parameter(torch.zeros(wshape[0]))
        w = torch.randn(wshape) * 0.01
        self.weight_orig = nn.Parameter(w)
        W = w.flatten(1)
        self.register_buffer('weight_u', F.normalize(torch.randn(W.shape[0]), dim=0, eps=eps))
        self.register_buffer('weight_v', F.normalize(torch.randn(W.shape[1]), dim=0, eps=eps))

    def weight(self):
        W = self.weight_orig.flatten(1)
        u, v = self.weight_u, self.weight_v
        if self.training:
            with torch.no_grad():
                v = F.normalize(torch.mv(W.t(), u), dim=0, eps=self.eps, out=v)
                u = F.normalize(torch.mv(W, v), dim=0, eps=self.eps, out=u)
            u, v = u.clone(memory_format=torch.contiguous_format), v.clone(memory_format=torch.contiguous_format)
        sigma = torch.dot(u, torch.mv(W, v))
        return self.weight_orig / sigma


class DiscriminatorS(_SingleDisc):
    """modules/hifigan/hifigan.py:253-286.  forward(x [B,1,T], mel=None) -> (out [B, L_7], fmap: eight maps [B, C, L_l]), differentiable with respect
    to x and every parameter.  convs[l] / conv_post hold bias and weight_g [Co,1,1], weight_v [Co,Ci/g,K] (or weight after remove_weight_norm());
    under use_spectral_norm weight_orig and the buffers weight_u, weight_v.  The normalisations are torch expressions."""

    def __init__(self, use_spectral_norm=False, use_cond=False, upsample_rates=None, c_in=1):
        super().__init__()
        bad = []
        if use_cond:
            bad.append('use_cond (the mel-conditioned input)')
        if c_in != 1:
            bad.append('c_in other than 1')
        if bad:
            raise NotImplementedError('DiscriminatorS on HIP covers the shipped configuration only: ' + '; '.join(bad))
        self.use_cond, self.use_spectral_norm = False, bool(use_spectral_norm)
        shapes = [(co, ci // g, k) for ci, co, k, _, g in _S_LAYERS]
        mods = [_SN(s) if use_spectral_norm else _WN(s, True, True, bias_first=True) for s in shapes]
        self.convs = nn.ModuleList(mods[:-1])
        self.conv_post = mods[-1]

    @staticmethod
    def _weight(m):
        return m.weight() if isinstance(m, _SN) else _SingleDisc._weight(m)

    def _check_device(self, x, who):
        p = self.conv_post.bias
        if p.device != x.device or p.dtype != torch.float32:
            raise ValueError(f'{who}: the parameters are {p.dtype} on {p.device}, x is on {x.device}')

    def forward(self, x, mel=None):
        self._refuse_mel(mel)
        _check_sx(x, 'DiscriminatorS')
        self._check_device(x, 'DiscriminatorS')
        ws, bs = self._params()
        return disc_s_op(x, ws, bs, LRELU_SLOPE)


class _MeanPool(nn.Module):
    """AvgPool1d(4, 2, padding=1) on avg_pool_op: a parameter-free member, as the reference's meanpools are"""

    def forward(self, x):
        return avg_pool_op(x)


class MultiScaleDiscriminator(_Disc):
    """modules/hifigan/hifigan.py:289-325: three DiscriminatorS, the first under spectral norm, behind cumulative AvgPool1d(4, 2, 1).  forward(y, y_hat,
    mel=None) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs); T >= 4.  The weight-normed discriminators run d(y) and d(y_hat) as one batch of 2 B; the
    spectral-normed one too in eval(), but in train() as two calls, y first: its buffers move between them, as in the reference."""

    def __init__(self, use_cond=False, c_in=1):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorS(use_spectral_norm=True, use_cond=use_cond, c_in=c_in),
                                             DiscriminatorS(use_cond=use_cond, c_in=c_in), DiscriminatorS(use_cond=use_cond, c_in=c_in)])
        self.meanpools = nn.ModuleList([_MeanPool(), _MeanPool()])

    def forward(self, y, y_hat, mel=None):
        self._refuse_mel(mel)
        _check_sx(y, 'MultiScaleDiscriminator', 4)
        _check_pair(y, y_hat, 'MultiScaleDiscriminator')
        if 2 * y.shape[0] > 65535:
            raise ValueError(f'MultiScaleDiscriminator: 2 B = {2 * y.shape[0]} exceeds 65535 rows')
        for d in self.discriminators:
            d._check_device(y, 'MultiScaleDiscriminator')
        yy = torch.cat([y, y_hat]).contiguous()
        rs, gs, frs, fgs = [], [], [], []
        for i, d in enumerate(self.discriminators):
            if i != 0:
                yy = self.meanpools[i - 1](yy)                  # the pooling is per row: the pair is pooled as one batch
            if d.use_spectral_norm and self.training:
                Bh = yy.shape[0] // 2
                r, fr = d(yy[:Bh])
                g, fg = d(yy[Bh:])
            else:
                ws, bs = d._params()
                _check_params(yy, ws, bs, LRELU_SLOPE, 'MultiScaleDiscriminator', _S_SHAPES, 'eight')
                (r, fr), (g, fg) = _disc_s_pair(yy, ws, bs, LRELU_SLOPE)
            rs.append(r); gs.append(g); frs.append(fr); fgs.append(fg)
        return rs, gs, frs, fgs


def hifigan_adversarial_losses(disc, y, y_hat):
    """the generator's terms against `disc` (a MultiPeriodDiscriminator or a MultiScaleDiscriminator): dict(adv = generator_loss(d(y_hat)), fm = feature_loss(fmaps of y, of
    y_hat)); gradients flow to y_hat (and to the discriminator's parameters, which a generator step does not update)"""
    _, gs, frs, fgs = disc(y, y_hat)
    return dict(adv=generator_loss(gs), fm=feature_loss(frs, fgs))


def hifigan_discriminator_losses(disc, y, y_hat):
    """the discriminator's pair (r_loss, g_loss) = discriminator_loss(d(y), d(y_hat.detach())) of `disc` (a MultiPeriodDiscriminator or a
    MultiScaleDiscriminator; the latter's spectral buffers advance once per d(.) call in train())"""
    rs, gs, _, _ = disc(y, y_hat.detach())
    return discriminator_loss(rs, gs)
