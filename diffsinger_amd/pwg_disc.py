"""ParallelWaveGAN discriminator and the LSGAN losses on the HIP operators of include/dsv.h, section "PWG discriminator" (kernels:
csrc/pwg_disc.hpp) - the adversarial half of the PWG trainer's objective (configs/tts/pwg.yaml: lambda_adv against discriminator_params).

    ParallelWaveGANDiscriminator   modules/parallel_wavegan/models/parallel_wavegan.py:207-300: the reference's constructor signature, defaults and
                                   state-dict keys (conv_layers.{0,2,...}.{weight_g,weight_v,bias}, or .weight after remove_weight_norm())
    pwg_disc_op                    the same network on plain weights, forward and backward through ONE autograd node
    lsgan_loss_op                  mean((d - target)^2)
    generator_loss, discriminator_loss      modules/hifigan/hifigan.py:359-365 and :337-347

Every convolution, its data / weight / bias gradients, the activation and its derivative, and the loss run in HIP; the weight-norm expression
g * v / ||v|| and its gradient stay torch expressions on [64][64][3] tensors.  torch is plumbing otherwise (buffers, streams, the autograd
graph).  There is no CPU path.  Nothing here synchronises or reads a device value on the host: after one warm-up call forward, loss and
backward record into one torch.cuda.graph on a single stream.

Kernel launches through the library are counted (`launch_count()`): a forward of an n-layer network is n + 3 (pad, pack + its slack fill, one
per layer), its backward 3 n (pad, three for the last layer, three per middle layer, two for the first) plus one when the input requires a
gradient; lsgan_loss_op is two forward and one backward."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .pwg import _WN
from .vocoder import padded_samples

__all__ = ['ParallelWaveGANDiscriminator', 'pwg_disc_op', 'lsgan_loss_op', 'generator_loss', 'discriminator_loss', 'launch_count']

_C = 64
_LAUNCHES = [0]


def launch_count() -> int:
    """kernels (and fills) launched through the library by this module since import"""
    return _LAUNCHES[0]


def _call(name, n, dev, *args):
    _lib.call(name, dev, *args)
    _LAUNCHES[0] += n


def _pad_rows(x2d: torch.Tensor, T: int) -> torch.Tensor:
    """[R][T] contiguous -> [R][LS], zero in [T, LS)"""
    R = x2d.shape[0]
    out = torch.empty(R, padded_samples(T), device=x2d.device, dtype=torch.float32)
    _call('dsv_pad_rows', 1, x2d.device, x2d.data_ptr(), out.data_ptr(), R, T)
    return out


class PwgDiscFunction(torch.autograd.Function):
    """x [B][1][T], n weights, n biases (None where the layer has none) -> p [B][1][T] (+ the n - 1 post-activations as [B][64][T] views)."""

    @staticmethod
    def forward(ctx, x, slope, n, return_saved, *params):
        lib = _lib.load()
        ws, bs = params[:n], params[n:]
        dev = x.device
        B, _, T = x.shape
        LS = padded_samples(T)
        xp = _pad_rows(x.reshape(B, T), T)
        # the middle layers' matrices, forward [co][tap * 64 + ci] and data gradient [ci][tap * 64 + co] = W[co][ci][2 - tap], packed by one call
        wall = torch.stack([w.detach() for w in ws[1:n - 1]])                                    # [n - 2][64][64][3]
        mats = torch.cat([wall.permute(0, 1, 3, 2).reshape(n - 2, _C, 3 * _C), wall.flip(3).permute(0, 2, 3, 1).reshape(n - 2, _C, 3 * _C)], 1)
        mats = mats.reshape((n - 2) * 2 * _C, 3 * _C).contiguous()
        rows = mats.shape[0]
        packed = torch.empty(lib.dsv_packed_floats(rows, 3 * _C, 1), device=dev, dtype=torch.float32)
        _call('dsv_pack_weight', 2, dev, mats.data_ptr(), rows, 3 * _C, 1, packed.data_ptr())
        w0, wl = ws[0].detach().contiguous(), ws[n - 1].detach().contiguous()
        b = [None if t is None else t.detach().contiguous() for t in bs]
        acts = [torch.empty(B, _C, LS, device=dev, dtype=torch.float32) for _ in range(n - 1)]
        _call('dsv_pwgd_first', 1, dev, xp.data_ptr(), w0.data_ptr(), _lib.ptr(b[0]), acts[0].data_ptr(), B, T, slope)
        for l in range(1, n - 1):
            off = (l - 1) * 2 * _C * 3 * _C * 4
            _call('dsv_pwgd_layer', 1, dev, acts[l - 1].data_ptr(), packed.data_ptr() + off, _lib.ptr(b[l]), None, acts[l].data_ptr(), B, T, l, slope, 0)
        p = torch.empty(B, LS, device=dev, dtype=torch.float32)
        _call('dsv_pwgd_last', 1, dev, acts[n - 2].data_ptr(), wl.data_ptr(), _lib.ptr(b[n - 1]), p.data_ptr(), B, T)
        ctx.save_for_backward(xp, packed, w0, wl, *acts)
        ctx.meta = (B, T, float(slope), n, [t is not None for t in bs])
        out = p[:, None, :T]
        if not return_saved:
            return out
        views = tuple(a[:, :, :T] for a in acts)
        ctx.mark_non_differentiable(*views)
        return (out,) + views

    @staticmethod
    @once_differentiable
    def backward(ctx, gp, *unused):
        lib = _lib.load()
        xp, packed, w0, wl, *acts = ctx.saved_tensors
        B, T, slope, n, has_b = ctx.meta
        dev = gp.device
        LS = padded_samples(T)
        g = _pad_rows(gp.to(torch.float32).reshape(B, T).contiguous(), T)
        ws_e = torch.empty(lib.dsv_pwgd_edge_workspace_floats(B, T), device=dev, dtype=torch.float32)
        ws_w = torch.empty(lib.dsv_pwgd_wgrad_workspace_floats(B, T), device=dev, dtype=torch.float32)
        dws: List[Optional[torch.Tensor]] = [None] * n
        dbs: List[Optional[torch.Tensor]] = [None] * n
        dws[n - 1] = torch.empty(1, _C, 3, device=dev, dtype=torch.float32)
        dbs[n - 1] = torch.empty(1, device=dev, dtype=torch.float32) if has_b[n - 1] else None
        G = torch.empty(B, _C, LS, device=dev, dtype=torch.float32)
        G2 = torch.empty_like(G)
        _call('dsv_pwgd_last_backward', 3, dev, g.data_ptr(), acts[n - 2].data_ptr(), wl.data_ptr(), ws_e.data_ptr(), dws[n - 1].data_ptr(),
              _lib.ptr(dbs[n - 1]), G.data_ptr(), B, T, slope)
        for l in range(n - 2, 0, -1):
            dws[l] = torch.empty(_C, _C, 3, device=dev, dtype=torch.float32)
            dbs[l] = torch.empty(_C, device=dev, dtype=torch.float32) if has_b[l] else None
            _call('dsv_pwgd_wgrad', 2, dev, G.data_ptr(), acts[l - 1].data_ptr(), ws_w.data_ptr(), dws[l].data_ptr(), _lib.ptr(dbs[l]), B, T, l)
            off = ((l - 1) * 2 + 1) * _C * 3 * _C * 4
            _call('dsv_pwgd_layer', 1, dev, G.data_ptr(), packed.data_ptr() + off, None, acts[l - 1].data_ptr(), G2.data_ptr(), B, T, l, slope, 1)
            G, G2 = G2, G
        dws[0] = torch.empty(_C, 1, 3, device=dev, dtype=torch.float32)
        dbs[0] = torch.empty(_C, device=dev, dtype=torch.float32) if has_b[0] else None
        dx = torch.empty(B, LS, device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        _call('dsv_pwgd_first_backward', 3 if dx is not None else 2, dev, G.data_ptr(), xp.data_ptr(), w0.data_ptr(), ws_e.data_ptr(), dws[0].data_ptr(),
              _lib.ptr(dbs[0]), _lib.ptr(dx), B, T)
        gx = None if dx is None else dx[:, None, :T]
        return (gx, None, None, None) + tuple(dws) + tuple(dbs)


def _check_x(x, who):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f'{who}: x must be a tensor')
    if x.dim() != 3 or x.shape[1] != 1 or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f'{who}: x must be [B][1][T] with B >= 1 and T >= 1, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        raise ValueError(f'{who}: x must be float32, got {x.dtype}')
    if not x.is_cuda:
        raise ValueError(f'{who}: x must be a device tensor (there is no CPU path), got {x.device}')
    if x.shape[0] > 65535:
        raise ValueError(f'{who}: x has B={x.shape[0]} > 65535 rows')


def pwg_disc_op(x, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]], slope: float, *, return_saved: bool = False):
    """The discriminator on plain weights: weights[0] [64][1][3], weights[1 .. n - 2] [64][64][3] (dilation = index), weights[n - 1] [1][64][3],
    biases[i] [Co] or None; x float32 [B][1][T] on the device -> [B][1][T].  return_saved=True: (out, [a_0 ... a_{n - 2}]), the saved
    post-activations as [B][64][T] views (no gradient flows through them)."""
    _check_x(x, 'pwg_disc_op')
    n = len(weights)
    if not 3 <= n <= 10 or len(biases) != n:
        raise ValueError(f'pwg_disc_op: 3 to 10 weights and as many biases (None where absent), got {n} and {len(biases)}')
    if not 0.0 < float(slope) < 1.0:
        raise ValueError(f'pwg_disc_op: slope={slope} must be in (0, 1)')
    for i, w in enumerate(weights):
        want = (_C, 1, 3) if i == 0 else (1, _C, 3) if i == n - 1 else (_C, _C, 3)
        if tuple(w.shape) != want or w.dtype != torch.float32 or w.device != x.device:
            raise ValueError(f'pwg_disc_op: weights[{i}] must be float32 {want} on {x.device}, got {w.dtype} {tuple(w.shape)} on {w.device}')
        bi = biases[i]
        if bi is not None and (tuple(bi.shape) != (want[0],) or bi.dtype != torch.float32 or bi.device != x.device):
            raise ValueError(f'pwg_disc_op: biases[{i}] must be float32 ({want[0]},) on {x.device}, got {bi.dtype} {tuple(bi.shape)} on {bi.device}')
    out = PwgDiscFunction.apply(x.contiguous(), float(slope), n, bool(return_saved), *weights, *biases)
    if return_saved:
        return out[0], list(out[1:])
    return out


class ParallelWaveGANDiscriminator(nn.Module):
    """modules/parallel_wavegan/models/parallel_wavegan.py:207-300.  forward(x [B,1,T]) -> [B,1,T], differentiable with respect to x and every
    parameter.  conv_layers[2 i] holds layer i's parameters (dilation 1 for the first and last, i for the others), conv_layers[2 i + 1] is the
    parameter-free activation."""

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1,
                 nonlinear_activation='LeakyReLU', nonlinear_activation_params={'negative_slope': 0.2}, bias=True, use_weight_norm=True):
        super().__init__()
        params = dict(nonlinear_activation_params or {})
        slope = params.pop('negative_slope', 0.01)
        params.pop('inplace', None)
        bad = []
        if (in_channels, out_channels, kernel_size) != (1, 1, 3):
            bad.append('in_channels / out_channels / kernel_size other than 1 / 1 / 3')
        if conv_channels != _C:
            bad.append('conv_channels other than 64')
        if dilation_factor != 1:
            bad.append('dilation_factor other than 1')
        if not isinstance(layers, int) or not 3 <= layers <= 10:
            bad.append('layers outside [3, 10]')
        if nonlinear_activation != 'LeakyReLU' or params or not 0.0 < float(slope) < 1.0:
            bad.append('an activation other than LeakyReLU with 0 < negative_slope < 1')
        if bad:
            raise NotImplementedError('ParallelWaveGANDiscriminator on HIP covers the shipped configuration only: ' + '; '.join(bad))
        self.layers, self.negative_slope = layers, float(slope)
        wn, bias = bool(use_weight_norm), bool(bias)
        mods = []
        for i in range(layers - 1):
            mods += [_WN((_C, 1 if i == 0 else _C, 3), bias, wn), nn.LeakyReLU(self.negative_slope)]
        mods.append(_WN((1, _C, 3), bias, wn))
        self.conv_layers = nn.ModuleList(mods)

    def remove_weight_norm(self):
        for m in self.modules():
            if isinstance(m, _WN):
                m.remove_weight_norm()

    def forward(self, x):
        _check_x(x, 'ParallelWaveGANDiscriminator')
        convs = [self.conv_layers[2 * i] for i in range(self.layers)]
        weights = [torch._weight_norm(m.weight_v, m.weight_g, 0) if hasattr(m, 'weight_g') else m.weight for m in convs]
        return pwg_disc_op(x, weights, [m.bias for m in convs], self.negative_slope)


class LsganFunction(torch.autograd.Function):
    """d float32 [n] contiguous -> 0-dim mean((d - target)^2)"""

    @staticmethod
    def forward(ctx, d, target):
        lib = _lib.load()
        n = d.numel()
        ws = torch.empty(lib.dsv_pwgd_lsgan_workspace_floats(n) // 2, device=d.device, dtype=torch.float64)
        out = torch.empty(1, device=d.device, dtype=torch.float32)
        _call('dsv_pwgd_lsgan', 2, d.device, d.data_ptr(), target, ws.data_ptr(), out.data_ptr(), n)
        ctx.save_for_backward(d)
        ctx.target = target
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        d, = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).contiguous()
        G = torch.empty_like(d)
        _call('dsv_pwgd_lsgan_backward', 1, d.device, d.data_ptr(), ctx.target, g.data_ptr(), G.data_ptr(), d.numel())
        return G, None


def lsgan_loss_op(d, target: float):
    """mean((d - target)^2) over every element of d (float32, on the device, any shape) -> 0-dim float32; float64 sums in a fixed order."""
    if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or not d.is_cuda or d.numel() < 1:
        what = f'{d.dtype} {tuple(d.shape)} on {d.device}' if isinstance(d, torch.Tensor) else type(d).__name__
        raise ValueError(f'lsgan_loss_op: d must be a non-empty float32 device tensor (there is no CPU path), got {what}')
    return LsganFunction.apply(d.contiguous().reshape(-1), float(target))


def generator_loss(disc_outputs):
    """modules/hifigan/hifigan.py:359-365: mean over the discriminators of mean((1 - D(G(z)))^2)."""
    loss = 0
    for dg in disc_outputs:
        loss = loss + lsgan_loss_op(dg, 1.0)
    return loss / len(disc_outputs)


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """modules/hifigan/hifigan.py:337-347: (mean of mean((1 - D(y))^2), mean of mean(D(G(z))^2)), both divided by the number of real outputs."""
    r_losses, g_losses = 0, 0
    for dr, dg in zip(disc_real_outputs, disc_generated_outputs):
        r_losses = r_losses + lsgan_loss_op(dr, 1.0)
        g_losses = g_losses + lsgan_loss_op(dg, 0.0)
    return r_losses / len(disc_real_outputs), g_losses / len(disc_real_outputs)
