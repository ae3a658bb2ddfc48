"""HiFi-GAN multi-scale discriminator, the pieces built so far, on the HIP operators of include/dsv.h, section "HiFi-GAN scale discriminator"
(kernels: csrc/hifigan_disc.hpp).

    avg_pool_op                                AvgPool1d(4, 2, padding=1) of MultiScaleDiscriminator (modules/hifigan/hifigan.py:304-307), forward
                                               and backward
    generator_loss, discriminator_loss         pwg_disc's (hifigan.py:337-347, :359-365); cond_discriminator_loss hifigan.py:350-356

DiscriminatorS itself - the grouped, strided Conv1d stack and the feature-matching loss - is not here: see DESIGN.md section 6 "HiFi-GAN scale
discriminator".  There is no CPU path.  Nothing here synchronises or reads a device value on the host.

Kernel launches through the library are counted by pwg_disc's counter (`launch_count()` is that function): avg_pool_op is one launch forward
and one backward - the kernels take the rows of a dense [B][T] tensor as they lie, no padding pass; lsgan_loss_op 2 forward, 1 backward."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .pwg_disc import _call, _check_x as _check_pwg_x, discriminator_loss, generator_loss, launch_count, lsgan_loss_op
from .vocoder import padded_samples

__all__ = ['avg_pool_op', 'generator_loss', 'discriminator_loss', 'cond_discriminator_loss', 'launch_count']


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
