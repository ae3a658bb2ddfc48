"""ParallelWaveGAN generator training on the HIP operators of include/dsv.h, section "PWG generator training" (kernels: csrc/pwg_train.hpp), and
the trainer's two objectives as thin compositions of the operators that already exist (stft_loss.py, pwg_disc.py).

    pwg_gen_op                     the generator on plain weights, forward and backward through ONE autograd node (PwgGenFunction);
                                   ParallelWaveGANGenerator.forward_train applies the weight-norm expression in torch and calls it
    pwg_generator_losses           sc + mag + lambda_adv * adv of configs/tts/pwg.yaml (stft_loss_params, lambda_adv, discriminator_params)
    pwg_discriminator_losses       the LSGAN pair on D(y) and D(G(z).detach())
    pwg_training_step              generator objective, backward, clip, optional step; from disc_start_steps on the same for the discriminator

The reference's tasks.vocoder.pwg.PwgTask is missing from the snapshot this package was written against: the composition here
is what the keys of configs/tts/pwg.yaml (stft_loss_params, lambda_adv, generator_grad_norm, discriminator_grad_norm, disc_start_steps) and the
LSGAN losses of modules/hifigan/hifigan.py:337-365 define.  The optimisers are arguments: voc_optim.pwg_optimizers builds the RAdam + StepLR
pairs the same file configures (optimizers/radam.py's arithmetic on HIP over the list of parameter tensors), and a step given one of those
clips and updates without reading the norm on the host; any other torch optimiser takes clip_grad_norm_ + step().

Saved state of one forward: per block its input x_l [B][64][LS] and the gate pre-activations a_l [B][128][LS] (the backward recomputes tanh,
sigmoid and z from a_l), the scaled skip sum, the hidden activation of last_conv_layers, the upsampled conditioning and each upsampling
stage's input.  Nothing here synchronises or reads a device value on the host: forward, objective and backward record into one
torch.cuda.graph on a single stream.  Every sum runs in a fixed order: two steps on the same inputs are bitwise equal."""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .pwg_disc import discriminator_loss, generator_loss
from .vocoder import padded_samples
from .voc_optim import MultiTensorOptimizer

__all__ = ['pwg_gen_op', 'pwg_generator_losses', 'pwg_discriminator_losses', 'pwg_training_step', 'launch_count']

_LAUNCHES = [0]


def launch_count() -> int:
    """kernels (and fills) launched through the library by this module since import"""
    return _LAUNCHES[0]


def _call(name, n, dev, *args):
    _lib.call(name, dev, *args)
    _LAUNCHES[0] += n


def _new(dev, *shape):
    return torch.empty(*shape, device=dev, dtype=torch.float32)


def _pad_rows(x: torch.Tensor) -> torch.Tensor:
    """[B][C][L] -> [B][C][LS], zero in [L, LS)"""
    B, C, L = x.shape
    x = x.contiguous()
    out = _new(x.device, B, C, padded_samples(L))
    _call('dsv_pad_rows', 1, x.device, x.data_ptr(), out.data_ptr(), B * C, L)
    return out


def _pack(mat: torch.Tensor) -> torch.Tensor:
    """dsv_pack_weight of a [rows][K] matrix"""
    lib = _lib.load()
    mat = mat.contiguous()
    rows, K = mat.shape
    buf = _new(mat.device, lib.dsv_packed_floats(rows, K, 1))
    _call('dsv_pack_weight', 2, mat.device, mat.data_ptr(), rows, K, 1, buf.data_ptr())
    return buf


def _conv(x, L, wp, bias, rows, ci, k, pre_slope=1.0):
    """dsv_conv1d without padding or dilation (the inference path's call for conv_in and last_conv_layers)"""
    out = _new(x.device, x.shape[0], rows, padded_samples(L))
    _call('dsv_conv1d', 1, x.device, x.data_ptr(), wp.data_ptr(), _lib.ptr(bias), out.data_ptr(), x.shape[0], ci, rows, k, 0, 1, L, 1, float(pre_slope),
          None, None, 1.0, 0)
    return out


class PwgGenFunction(torch.autograd.Function):
    """x [B][1][T], c [B][aux][T / hop + 2 ctx], meta, plain parameters -> y [B][1][T].  The parameters, in order: first_conv weight, bias;
    conv_in weight; one smoothing filter per upsampling stage; per block conv weight, conv bias, conv1x1_aux weight, conv1x1_out weight, bias,
    conv1x1_skip weight, bias; last_conv_layers[1] weight, bias; last_conv_layers[3] weight, bias.  A bias the module does not have is None."""

    @staticmethod
    def forward(ctx, x, c, meta, *params):
        dev = x.device
        aux, kin, scales, dils = meta['aux'], meta['k_in'], meta['scales'], meta['dilations']
        nl, ns = len(dils), len(scales)
        pd = [None if p is None else p.detach().contiguous() for p in params]
        w0, b0, w_in = pd[0], pd[1], pd[2]
        filts = pd[3:3 + ns]
        blocks = [pd[3 + ns + 7 * i:3 + ns + 7 * (i + 1)] for i in range(nl)]
        wl1, bl1, wl3, bl3 = pd[3 + ns + 7 * nl:]
        B, _, T = x.shape
        Tc = c.shape[2]
        LS = padded_samples(T)
        # ConvInUpsampleNetwork: conv_in without padding, then the stretch + smoothing stages; every stage's input is kept
        cpad = _pad_rows(c.to(torch.float32))
        wp_in = torch.empty(_lib.load().dsv_packed_floats(aux, aux, kin), device=dev, dtype=torch.float32)
        _call('dsv_pack_weight', 2, dev, w_in.data_ptr(), aux, aux, kin, wp_in.data_ptr())
        y = _conv(cpad, Tc, wp_in, None, aux, aux, kin)
        L = Tc - (kin - 1)
        y = _pad_rows(y[:, :, :L])
        ups_in = []
        for f, sc in zip(filts, scales):
            ups_in.append(y)
            out = _new(dev, B, aux, padded_samples(L * sc))
            _call('dsv_pwg_upsample', 1, dev, y.data_ptr(), f.data_ptr(), out.data_ptr(), B * aux, L, sc)
            y, L = out, L * sc
        if L != T:
            raise ValueError(f'forward_train: the conditioning upsamples to {L} samples, the noise has {T}')
        z = _pad_rows(x.to(torch.float32))
        xs = [_new(dev, B, 64, LS)]
        _call('dsv_pwg_first', 1, dev, z.data_ptr(), w0.data_ptr(), b0.data_ptr(), xs[0].data_ptr(), B, 64, T)
        # every block's two matrices, packed by one call each: [nl * 128][192 + aux] (columns tap * 64 + ci, then the aux channels), [nl * 128][64]
        m1 = torch.cat([torch.cat([blk[0].permute(0, 2, 1).reshape(128, 192), blk[2][:, :, 0]], 1) for blk in blocks], 0)
        m2 = torch.cat([torch.cat([blk[3][:, :, 0], blk[5][:, :, 0]], 0) for blk in blocks], 0)
        p1, p2 = _pack(m1), _pack(m2)
        n1 = 192 + aux
        skips = _new(dev, B, 64, LS)
        acts = []
        for i, (blk, dil) in enumerate(zip(blocks, dils)):
            b2 = None if blk[4] is None else torch.cat([blk[4], blk[6]])
            a, xo = _new(dev, B, 128, LS), _new(dev, B, 64, LS)
            _call('dsv_pwgt_layer', 1, dev, xs[i].data_ptr(), y.data_ptr(), p1.data_ptr() + 4 * i * (n1 // 8) * 256 * 4, _lib.ptr(blk[1]),
                  p2.data_ptr() + 4 * i * 8 * 256 * 4, _lib.ptr(b2), xo.data_ptr(), skips.data_ptr(), a.data_ptr(), B, T, aux, dil, 1 if i == 0 else 0)
            acts.append(a)
            xs.append(xo)
        S = skips * math.sqrt(1.0 / nl)
        o1 = _conv(S, T, _pack(wl1[:, :, 0]), bl1, 64, 64, 1, pre_slope=0.0)
        o = _conv(o1, T, _pack(wl3[:, :, 0]), bl3, 1, 64, 1, pre_slope=0.0)
        ctx.save_for_backward(cpad, y, z, S, o1, wl1, wl3, *filts, *ups_in, *xs[:nl], *acts, *[blk[j] for blk in blocks for j in (0, 2, 3, 5)])
        ctx.meta = (meta, B, T, Tc, [blk[1] is not None for blk in blocks])
        out = o[:, :, :T]
        if not meta.get('return_saved'):
            return out
        views = (S[:, :, :T], o1[:, :, :T])                    # the inputs of the two ReLUs of last_conv_layers (their masks are taken from these)
        ctx.mark_non_differentiable(*views)
        return (out,) + views

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, *unused):
        lib = _lib.load()
        meta, B, T, Tc, has_b = ctx.meta
        aux, kin, scales, dils = meta['aux'], meta['k_in'], meta['scales'], meta['dilations']
        nl, ns = len(dils), len(scales)
        sv = list(ctx.saved_tensors)
        cpad, y, z, S, o1, wl1, wl3 = sv[:7]
        filts, ups_in = sv[7:7 + ns], sv[7 + ns:7 + 2 * ns]
        xs, acts = sv[7 + 2 * ns:7 + 2 * ns + nl], sv[7 + 2 * ns + nl:7 + 2 * ns + 2 * nl]
        bw = sv[7 + 2 * ns + 2 * nl:]
        blocks = [bw[4 * i:4 * i + 4] for i in range(nl)]                                   # conv, aux, out, skip weights
        dev = gy.device
        LS = padded_samples(T)
        n1 = 192 + aux
        g = _pad_rows(gy.to(torch.float32).reshape(B, 1, T))
        ws = _new(dev, lib.dsv_pwgt_wgrad_workspace_floats(B, T, n1))
        # last_conv_layers: ReLU -> 1x1 (64 -> 64) -> ReLU -> 1x1 (64 -> 1)
        rd3 = _new(dev, 128)
        _call('dsv_pwgt_rowdot', 1, dev, g.data_ptr(), o1.data_ptr(), rd3.data_ptr(), B, 64, T, 0, 1, 1)
        d_wl3, d_bl3 = rd3[0::2].reshape(1, 64, 1), rd3[1:2]
        d_o1 = _new(dev, B, 64, LS)
        _call('dsv_pwgt_last_dgrad', 1, dev, g.data_ptr(), o1.data_ptr(), wl3.data_ptr(), d_o1.data_ptr(), B, 64, T)
        wg1 = _new(dev, 128 * 64 + 128)
        _call('dsv_pwgt_wgrad_relu', 2, dev, d_o1.data_ptr(), S.data_ptr(), ws.data_ptr(), wg1.data_ptr(), B, T)
        d_wl1, d_bl1 = wg1[:64 * 64].reshape(64, 64, 1), wg1[128 * 64:128 * 64 + 64]
        gS = _conv(d_o1, T, _pack(wl1[:, :, 0].t()), None, 64, 64, 1)
        dS = _new(dev, B, 64, LS)
        _call('dsv_pwgt_relu_mask', 1, dev, gS.data_ptr(), S.data_ptr(), dS.data_ptr(), math.sqrt(1.0 / nl), B * 64, T)
        # the transposed matrices of every block, packed by one call each
        w2t = _pack(torch.cat([torch.cat([blk[3][:, :, 0].t(), blk[2][:, :, 0].t()], 1) for blk in blocks], 0))          # [nl * 64][128]
        w1t = _pack(torch.cat([blk[0].permute(1, 2, 0).reshape(64, 384) for blk in blocks], 0))                          # [nl * 64][384]
        R = (aux + 31) // 32 * 32
        wat = _pack(torch.cat([torch.nn.functional.pad(blk[1][:, :, 0].t(), (0, 0, 0, R - aux)) for blk in blocks], 0))  # [nl * R][128]
        dC = _new(dev, B, aux, LS)
        da = _new(dev, B, 128, LS)
        dxb = [_new(dev, B, 64, LS), _new(dev, B, 64, LS)]
        dxp = None
        grads = []
        for i in range(nl - 1, -1, -1):
            a = acts[i]
            _call('dsv_pwgt_gate_backward', 1, dev, _lib.ptr(dxp), dS.data_ptr(), a.data_ptr(), w2t.data_ptr() + 2 * i * 16 * 256 * 4, da.data_ptr(), B, T)
            o2, o1g = _new(dev, 128 * 64 + 128), _new(dev, 128 * n1 + 128)
            _call('dsv_pwgt_wgrad_out', 2, dev, _lib.ptr(dxp), dS.data_ptr(), a.data_ptr(), ws.data_ptr(), o2.data_ptr(), B, T)
            _call('dsv_pwgt_wgrad_conv', 2, dev, da.data_ptr(), xs[i].data_ptr(), y.data_ptr(), ws.data_ptr(), o1g.data_ptr(), B, T, aux, dils[i])
            dxn = dxb[i & 1]
            _call('dsv_pwgt_conv_backward', 1, dev, da.data_ptr(), _lib.ptr(dxp), w1t.data_ptr() + 2 * i * 48 * 256 * 4,
                  wat.data_ptr() + (R // 32) * i * 16 * 256 * 4, dxn.data_ptr(), dC.data_ptr(), B, T, aux, dils[i], 1 if i == nl - 1 else 0)
            m1 = o1g[:128 * n1].reshape(128, n1)
            m2 = o2[:128 * 64].reshape(128, 64)
            last = dxp is None                                                               # its residual output is never read: no gradient
            hb = has_b[i]
            grads.append((m1[:, :192].reshape(128, 3, 64).permute(0, 2, 1).contiguous(), o1g[128 * n1:] if hb else None,
                          m1[:, 192:].reshape(128, aux, 1).contiguous(),
                          None if last else m2[:64].reshape(64, 64, 1), None if last or not hb else o2[128 * 64:128 * 64 + 64],
                          m2[64:].reshape(64, 64, 1), o2[128 * 64 + 64:] if hb else None))
            dxp = dxn
        grads.reverse()
        rd0 = _new(dev, 128)
        _call('dsv_pwgt_rowdot', 1, dev, dxp.data_ptr(), z.data_ptr(), rd0.data_ptr(), B, 64, T, 1, 0, 0)
        d_w0, d_b0 = rd0[0::2].reshape(64, 1, 1), rd0[1::2]
        # the upsampling network, last stage first
        gc, d_f = dC, [None] * ns
        for i in range(ns - 1, -1, -1):
            sc = scales[i]
            L_in = T
            for s2 in scales[i:]:
                L_in //= s2
            wsu = torch.empty(lib.dsv_pwgt_upsample_workspace_floats(B * aux, sc) // 2, device=dev, dtype=torch.float64)
            din = _new(dev, B, aux, padded_samples(L_in))
            d_f[i] = _new(dev, 1, 1, 1, 2 * sc + 1)
            _call('dsv_pwgt_upsample_backward', 3, dev, gc.data_ptr(), ups_in[i].data_ptr(), filts[i].data_ptr(), wsu.data_ptr(), din.data_ptr(),
                  d_f[i].data_ptr(), B * aux, L_in, sc)
            gc = din
        d_win = _new(dev, aux, aux, kin)
        _call('dsv_pwgt_convin_wgrad', 1, dev, gc.data_ptr(), cpad.data_ptr(), d_win.data_ptr(), B, aux, kin, Tc - (kin - 1))
        flat = [d_w0, d_b0, d_win] + d_f
        for gset in grads:
            flat += list(gset)
        flat += [d_wl1, d_bl1, d_wl3, d_bl3]
        return (None, None, None) + tuple(flat)


def pwg_gen_op(x, c, meta, params, *, return_saved=False):
    """The generator on plain weights (PwgGenFunction's parameter order); x float32 [B][1][T], c [B][aux][T / hop + 2 ctx] on the device.
    return_saved=True: (y, [S, o1]) - the scaled skip sum and the hidden activation of last_conv_layers as [B][64][T] views (no gradient flows
    through them): the inputs of the network's two ReLUs, whose masks the backward takes from these float32 values."""
    if not return_saved:
        return PwgGenFunction.apply(x, c, meta, *params)
    out = PwgGenFunction.apply(x, c, dict(meta, return_saved=True), *params)
    return out[0], list(out[1:])


def pwg_generator_losses(gen, disc, stft, x, c, y, *, lambda_adv, adversarial):
    """The generator's objective: y_ = gen.forward_train(x, c); sc, mag = stft(y_, y) (MultiResolutionSTFTLoss on [B][T]); when `adversarial`,
    adv = generator_loss([disc(y_)]) (mean((1 - D(G(z)))^2)); total = sc + mag + lambda_adv * adv.  -> (dict(total, sc, mag[, adv]), y_)"""
    y_ = gen.forward_train(x, c)
    sc, mag = stft(y_.squeeze(1), y.squeeze(1))
    losses = {'sc': sc, 'mag': mag}
    total = sc + mag
    if adversarial:
        adv = generator_loss([disc(y_)])
        losses['adv'] = adv
        total = total + lambda_adv * adv
    losses['total'] = total
    return losses, y_


def pwg_discriminator_losses(disc, y, y_):
    """discriminator_loss([disc(y)], [disc(y_.detach())]) -> dict(real, fake, total)"""
    real, fake = discriminator_loss([disc(y)], [disc(y_.detach())])
    return {'real': real, 'fake': fake, 'total': real + fake}


def _clip_and_step(params, max_norm, opt):
    """clip_grad_norm_(params, max_norm) and opt.step() when an optimiser is given -> the norm before clipping.  A MultiTensorOptimizer does
    both itself, over ITS parameters (the trainer builds it on `params`)."""
    if isinstance(opt, MultiTensorOptimizer):
        return opt.clip_and_step(max_norm)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    if opt is not None:
        opt.step()
    return norm


def pwg_training_step(gen, disc, stft, batch, hp, global_step, opt_g=None, opt_d=None):
    """One step of the ParallelWaveGAN trainer as configs/tts/pwg.yaml defines it.  batch = dict(x noise [B][1][T], c padded mel, y target
    [B][1][T]); hp holds lambda_adv, generator_grad_norm, discriminator_grad_norm, disc_start_steps.  The generator objective (adversarial from
    disc_start_steps on) and its backward, clip_grad_norm_ at generator_grad_norm, opt_g.step() when given; from disc_start_steps on the
    discriminator objective on the detached waveform, its backward, the clip at discriminator_grad_norm and opt_d.step().  An optimiser that
    is a voc_optim.MultiTensorOptimizer does clip and step in one go (clip_and_step: no host synchronisation; .grad stays unscaled).  Gradients
    are zeroed here before each backward (set_to_none).  -> dict of the loss terms plus the two pre-clip gradient norms."""
    adversarial = global_step >= hp['disc_start_steps']
    x, c, y = batch['x'], batch['c'], batch['y']
    gparams = [p for p in gen.parameters() if p.requires_grad]
    dparams = [p for p in disc.parameters() if p.requires_grad]
    for p in gparams + dparams:
        p.grad = None
    losses, y_ = pwg_generator_losses(gen, disc, stft, x, c, y, lambda_adv=hp['lambda_adv'], adversarial=adversarial)
    losses['total'].backward()
    out = {'gen_' + k: v.detach() for k, v in losses.items()}
    out['gen_grad_norm'] = _clip_and_step(gparams, hp['generator_grad_norm'], opt_g)
    if adversarial:
        for p in dparams:                                       # the generator's adversarial term left gradients here
            p.grad = None
        dl = pwg_discriminator_losses(disc, y, y_)
        dl['total'].backward()
        out.update({'disc_' + k: v.detach() for k, v in dl.items()})
        out['disc_grad_norm'] = _clip_and_step(dparams, hp['discriminator_grad_norm'], opt_d)
    return out
