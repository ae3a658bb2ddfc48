"""HiFi-GAN / NSF-HiFi-GAN generator training on the HIP operators of include/dsv.h, section "HiFi-GAN generator training" (kernels:
csrc/hifigan_train.hpp).

    hifigan_gen_op      the generator on plain weights, forward and backward through ONE autograd node (HifiGanGenFunction);
                        HifiGanGenerator.forward_train applies the weight-norm expression in torch and calls it
    hifigan_generator_losses, hifigan_generator_step
                        the mel term of the generator objective (lambda_mel * HifiGanMelLoss, diffsinger_amd/mel_loss.py) and one step on it
    hifigan_training_step
                        the full step: lambda_mel * mel + the adversarial and feature-matching terms against a list of discriminators
                        (diffsinger_amd/hifigan_disc.py), then the discriminators' objective on the detached waveform; optimisers:
                        diffsinger_amd/voc_optim.py (AdamW with adam_b1 / adam_b2) or any torch optimiser

The forward is the inference path's one-launch-per-convolution form (dsv_conv1d / dsv_conv1d_folded, bit-identical to the fused chains, DESIGN.md
section 6): every convolution's input is a tensor in memory and the leaky ReLU in front of it is applied while the kernel stages it, so the saved
pre-activations are buffers the forward writes anyway.  Weights are packed from the CURRENT parameters on every call (no cache: a captured step
replays the packing with it).

Saved state of one forward: the padded mel, the input of every convolution (one [B][C][LS] tensor per leaky ReLU), the padded output, and for
NSF the harmonic source `har` [B][LS] and the mixed sines [B][L][9].  Nothing here synchronises or reads a device value on the host, and
everything is enqueued on the current stream in one order: forward, objective and backward record into one torch.cuda.graph on a single stream.
Every sum runs in a fixed order: two steps on the same inputs are bitwise equal."""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .voc_optim import MultiTensorOptimizer
from .vocoder import LRELU_SLOPE, MAX_REACH, _HipOps, fold_weight, get_padding, padded_samples, polyphase_weight

__all__ = ['hifigan_gen_op', 'param_layout', 'hifigan_generator_losses', 'hifigan_generator_step', 'hifigan_training_step']

POST_SLOPE = 0.01                  # F.leaky_relu's default slope in front of conv_post (hifigan.py:167)
SINE_AMP, NOISE_STD, VOICED_THRESHOLD = 0.1, 0.003, 0.0

_OPS = [None]


def _ops() -> _HipOps:
    if _OPS[0] is None:
        _OPS[0] = _HipOps()
    return _OPS[0]


def _floats(dev, n: int) -> torch.Tensor:
    """a buffer of exactly the length one of the library's sizing functions returned"""
    if n < 0:
        raise ValueError('hifigan_train: the library refused the shape (a sizing function returned -1)')
    return torch.empty(int(n), device=dev, dtype=torch.float32)


def _act(dev, B, C, L) -> torch.Tensor:
    return _floats(dev, _lib.load().dsv_hgt_act_floats(B, C, L)).view(B, C, padded_samples(L))


def polyphase_taps(k: int, u: int):
    """The tap map of vocoder.polyphase_weight for ConvTranspose1d(kernel k, stride u, padding (k - u) / 2): per original tap j the output phase
    r[j] and the column t[j] of the polyphase filter it sits in, the polyphase kernel size and its padding."""
    p = (k - u) // 2
    r_of, d_of = [0] * k, [0] * k
    for r in range(u):
        s, m = r + p, 0
        while (s % u) + u * m < k:
            r_of[(s % u) + u * m], d_of[(s % u) + u * m] = r, s // u - m
            m += 1
    dmin, dmax = min(d_of), max(d_of)
    return r_of, [d - dmin for d in d_of], dmax - dmin + 1, -dmin


def param_layout(h):
    """Parameter holders of HifiGanGenerator in HifiGanGenFunction's order: [(prefix, kind)] with kind in 'pre', 'lin', 'up', 'noise', 'res', 'post';
    every holder contributes (plain weight, bias)."""
    rates = list(h['upsample_rates'])
    nk = len(h['resblock_kernel_sizes'])
    out = [('conv_pre.', 'pre')]
    if h.get('use_pitch_embed'):
        out.append(('m_source.l_linear.', 'lin'))
    for i in range(len(rates)):
        out.append((f'ups.{i}.', 'up'))
        if h.get('use_pitch_embed'):
            out.append((f'noise_convs.{i}.', 'noise'))
    for i in range(len(rates)):
        for j in range(nk):
            nd = 3 if str(h['resblock']) == '1' else 2
            for q in range(min(nd, len(h['resblock_dilation_sizes'][j]))):
                if str(h['resblock']) == '1':
                    out += [(f'resblocks.{i * nk + j}.convs1.{q}.', 'res'), (f'resblocks.{i * nk + j}.convs2.{q}.', 'res')]
                else:
                    out.append((f'resblocks.{i * nk + j}.convs.{q}.', 'res'))
    return out + [('conv_post.', 'post')]


def _fconv(ops, x, L, w, b, dil=1, **kw):
    """HifiGanGenerator._conv on a plain weight, packed here: the same kernel choice (the folded kernel for the narrow layers), the same bits"""
    co, ci, k = w.shape
    if get_padding(k, dil) > MAX_REACH:
        raise NotImplementedError(f'Conv1d kernel {k} at dilation {dil} reaches {get_padding(k, dil)} samples; the vocoder kernels stage +-{MAX_REACH}')
    F = ops.fold_factor(co, ci, k, dil)
    if F > 1:
        return ops.conv_folded(x, L, ops.pack(fold_weight(w, F)), b, co, ci, k, F, dil, **kw)
    return ops.conv(x, L, ops.pack(w), b, co, ci, k, get_padding(k, dil), dil, **kw)


class HifiGanGenFunction(torch.autograd.Function):
    """x [B][80][T], f0 [B][T] or None, rand_ini [B][9] / noise [B][T hop][9] or None, meta, then (plain weight, bias) per holder of
    param_layout(h) -> y [B][1][T hop] (+ the saved leaky-ReLU inputs and the mixed sines when meta['return_saved'])."""

    @staticmethod
    def forward(ctx, x, f0, rand_ini, noise, meta, *params):
        h = meta['h']
        ops, lib, dev = _ops(), _lib.load(), x.device
        layout = param_layout(h)
        pd = {}
        for n, (pre, _) in enumerate(layout):
            pd[pre] = (params[2 * n].detach().to(torch.float32).contiguous(), params[2 * n + 1].detach().to(torch.float32).contiguous())
        rates, ksz = list(h['upsample_rates']), list(h['upsample_kernel_sizes'])
        nk, kind = len(h['resblock_kernel_sizes']), str(h['resblock'])
        hop = int(np.prod(rates))
        B, M, T = x.shape
        xin = ops.pad_rows(x.detach().to(torch.float32).contiguous())
        har = sines = None
        Lh = T * hop
        if f0 is not None:
            H = pd['m_source.l_linear.'][0].numel()
            f0c = f0.detach().to(torch.float32).contiguous()
            nz = noise.detach().to(torch.float32).contiguous()
            ri = rand_ini.detach().to(torch.float32).contiguous()
            sw = torch.empty(B, H, Lh, device=dev, dtype=torch.float32)
            har = _act(dev, B, 1, Lh).view(B, -1)
            lw, lb = pd['m_source.l_linear.']
            _lib.call('dsv_sine_source', dev, f0c.data_ptr(), ri.data_ptr(), nz.data_ptr(), lw.reshape(-1).data_ptr(), lb.data_ptr(), sw.data_ptr(),
                  har.data_ptr(), B, T, hop, H, float(h['audio_sample_rate']), SINE_AMP, NOISE_STD, VOICED_THRESHOLD)
            sines = torch.empty(B, Lh, H, device=dev, dtype=torch.float32)
            _lib.call('dsv_hgt_source_mix', dev, f0c.data_ptr(), sw.data_ptr(), nz.data_ptr(), sines.data_ptr(), B, T, hop, H, SINE_AMP, NOISE_STD,
                  VOICED_THRESHOLD)
        L = T
        y = _fconv(ops, xin, L, *pd['conv_pre.'])
        pre = []                                                     # (saved input of a leaky ReLU, its length), in call order
        for i, (u, k) in enumerate(zip(rates, ksz)):
            xs = None
            if har is not None:
                nw, nb = pd[f'noise_convs.{i}.']
                s = int(np.prod(rates[i + 1:])) if i + 1 < len(rates) else 1
                xs = ops.noise_conv(har, Lh, nw[:, 0].contiguous(), nb, s, s // 2 if i + 1 < len(rates) else 0, L * u)
            pre.append((y, L))
            uw, ub = pd[f'ups.{i}.']
            wp, ppad = polyphase_weight(uw, u, (k - u) // 2)
            y = ops.conv(y, L, ops.pack(wp), ub, wp.shape[0], wp.shape[1], wp.shape[2], ppad, 1, up=u, pre_slope=LRELU_SLOPE, residual=xs)
            L = L * u
            acc = None
            for j in range(nk):
                dils = tuple(h['resblock_dilation_sizes'][j])[:3 if kind == '1' else 2]
                z = y
                for q, d in enumerate(dils):
                    last = q == len(dils) - 1
                    tail = dict(sum_in=acc if last else None, divide=float(nk) if (last and j == nk - 1) else 1.0)
                    pre.append((z, L))
                    if kind == '1':
                        xt = _fconv(ops, z, L, *pd[f'resblocks.{i * nk + j}.convs1.{q}.'], dil=d, pre_slope=LRELU_SLOPE)
                        pre.append((xt, L))
                        z = _fconv(ops, xt, L, *pd[f'resblocks.{i * nk + j}.convs2.{q}.'], dil=1, pre_slope=LRELU_SLOPE, residual=z, **tail)
                    else:
                        z = _fconv(ops, z, L, *pd[f'resblocks.{i * nk + j}.convs.{q}.'], dil=d, pre_slope=LRELU_SLOPE, residual=z, **tail)
                acc = z
            y = acc
        pre.append((y, L))
        o = _fconv(ops, y, L, *pd['conv_post.'], pre_slope=POST_SLOPE, act=1)
        weights = [pd[p][0] for p, kd in layout if kd in ('up', 'noise', 'res', 'post')]
        ctx.save_for_backward(xin, o, *[t for t, _ in pre], *weights, *([har, sines] if har is not None else []))
        ctx.meta = (h, B, T, len(pre), len(weights), har is not None)
        out = o[:, :, :L].contiguous()
        if not meta.get('return_saved'):
            return out
        views = tuple(t[:, :, :n] for t, n in pre) + ((sines,) if sines is not None else ())
        ctx.mark_non_differentiable(*views)
        return (out,) + views

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, *unused):
        lib = _lib.load()
        h, B, T, npre, nw, nsf = ctx.meta
        ops, dev = _ops(), gy.device
        sv = list(ctx.saved_tensors)
        xin, o = sv[0], sv[1]
        pre = sv[2:2 + npre]
        layout = param_layout(h)
        wts = dict(zip([p for p, kd in layout if kd in ('up', 'noise', 'res', 'post')], sv[2 + npre:2 + npre + nw]))
        har, sines = (sv[2 + npre + nw:] if nsf else (None, None))
        rates, ksz = list(h['upsample_rates']), list(h['upsample_kernel_sizes'])
        nk, kind = len(h['resblock_kernel_sizes']), str(h['resblock'])
        c0 = int(h['upsample_initial_channel'])
        hop = int(np.prod(rates))
        Lh = T * hop
        grads = {}
        # ONE workspace for every weight gradient of the step: the largest requirement, from the library's own sizing function
        need = [lib.dsv_hgt_wgrad_workspace_floats(B, T, c0, xin.shape[1], 7, 1)]
        L, ch = T, c0
        for i, (u, k) in enumerate(zip(rates, ksz)):
            need.append(lib.dsv_hgt_wgrad_workspace_floats(B, L, ch // 2, ch, polyphase_taps(k, u)[2], u))
            L, ch = L * u, ch // 2
            need += [lib.dsv_hgt_wgrad_workspace_floats(B, L, ch, ch, kk, 1) for kk in h['resblock_kernel_sizes']]
        need.append(lib.dsv_hgt_wgrad_workspace_floats(B, L, 1, ch, 7, 1))
        ws = _floats(dev, min(need) if min(need) < 0 else max(need))
        # ... and ONE for every bias sum: the widest layer of each rate
        bneed = [lib.dsv_hgt_bias_workspace_floats(B, c0, T), lib.dsv_hgt_bias_workspace_floats(B, 1, Lh)]
        L, ch = T, c0
        for u in rates:
            L, ch = L * u, ch // 2
            bneed.append(lib.dsv_hgt_bias_workspace_floats(B, ch, L))
        bws = _floats(dev, min(bneed) if min(bneed) < 0 else max(bneed))

        def conv_bwd(prefix, g, xs, w, L, dil, slope, residual=None, sum_in=None, divide=1.0, need_dx=True):
            """weight, bias and data gradient of one Conv1d behind a leaky ReLU; w None: no data gradient (conv_pre)"""
            co, ci, k = (w.shape if w is not None else (g.shape[1], xs.shape[1], 7))
            pad = get_padding(k, dil)
            dwk = _floats(dev, co * k * ci)
            _lib.call('dsv_hgt_conv_wgrad', dev, g.data_ptr(), xs.data_ptr(), ws.data_ptr(), ws.numel(), dwk.data_ptr(), B, co, ci, k, pad, dil, L, 1,
                  float(slope))
            db = _floats(dev, co)
            _lib.call('dsv_hgt_bias_grad', dev, g.data_ptr(), bws.data_ptr(), bws.numel(), db.data_ptr(), B, co, L)
            grads[prefix] = (dwk.view(co, k, ci).permute(0, 2, 1).contiguous(), db)
            if not need_dx:
                return None
            dx = _act(dev, B, ci, L)
            wt = ops.pack(w.flip(2).transpose(0, 1).contiguous())
            _lib.call('dsv_hgt_conv_dgrad', dev, g.data_ptr(), wt.data_ptr(), xs.data_ptr(), _lib.ptr(residual), _lib.ptr(sum_in), dx.data_ptr(), B, co, ci, k, pad,
                  dil, L, float(slope), float(divide))
            return dx

        L = Lh
        gp = _act(dev, B, 1, L)
        _lib.call('dsv_hgt_tanh_backward', dev, gy.to(torch.float32).contiguous().data_ptr(), o.data_ptr(), gp.data_ptr(), B, L)
        G = conv_bwd('conv_post.', gp, pre[-1], wts['conv_post.'], L, 1, POST_SLOPE, divide=float(nk))
        npair = 2 if kind == '1' else 1
        per_rb = [len(tuple(h['resblock_dilation_sizes'][j])[:3 if kind == '1' else 2]) for j in range(nk)]
        per_stage = 1 + npair * sum(per_rb)
        dhar = _act(dev, B, 1, Lh).view(B, -1) if nsf else None
        first_noise = True
        for i in range(len(rates) - 1, -1, -1):
            u, k = rates[i], ksz[i]
            ch = c0 // 2 ** (i + 1)
            base = i * per_stage
            din = None                                               # running sum of the parallel resblocks' input gradients, j ascending
            off = base + 1
            for j in range(nk):
                dils = tuple(h['resblock_dilation_sizes'][j])[:3 if kind == '1' else 2]
                gz = G
                for q in range(len(dils) - 1, -1, -1):
                    head = dict(residual=gz, sum_in=din if q == 0 else None)
                    if kind == '1':
                        z, xt = pre[off + 2 * q], pre[off + 2 * q + 1]
                        p1, p2 = f'resblocks.{i * nk + j}.convs1.{q}.', f'resblocks.{i * nk + j}.convs2.{q}.'
                        dxt = conv_bwd(p2, gz, xt, wts[p2], L, 1, LRELU_SLOPE)
                        gz = conv_bwd(p1, dxt, z, wts[p1], L, dils[q], LRELU_SLOPE, **head)
                    else:
                        p1 = f'resblocks.{i * nk + j}.convs.{q}.'
                        gz = conv_bwd(p1, gz, pre[off + q], wts[p1], L, dils[q], LRELU_SLOPE, **head)
                din = gz
                off += npair * len(dils)
            Gin = din                                                # the gradient at ups.i's output (+ noise_convs.i's)
            if nsf:
                nwt = wts[f'noise_convs.{i}.']
                C, K = nwt.shape[0], nwt.shape[2]
                s = int(np.prod(rates[i + 1:])) if i + 1 < len(rates) else 1
                dnw, dnb = _floats(dev, C * K), _floats(dev, C)
                _lib.call('dsv_hgt_noise_conv_backward', dev, Gin.data_ptr(), har.data_ptr(), nwt.reshape(C, K).contiguous().data_ptr(), bws.data_ptr(),
                      bws.numel(), dnw.data_ptr(), dnb.data_ptr(), dhar.data_ptr(), B, C, K, s, s // 2 if i + 1 < len(rates) else 0, Lh, L, 1 if first_noise else 0)
                first_noise = False
                grads[f'noise_convs.{i}.'] = (dnw.view(C, 1, K), dnb)
            # ups.i: the weight gradient through the forward's polyphase view (rows co * u + phase at the input rate), the data gradient as a gather
            uw = wts[f'ups.{i}.']
            ci, co = uw.shape[0], uw.shape[1]
            L_in = L // u
            r_of, t_of, kk, ppad = polyphase_taps(k, u)
            dwp = _floats(dev, co * u * kk * ci)
            xup = pre[base]
            _lib.call('dsv_hgt_conv_wgrad', dev, Gin.data_ptr(), xup.data_ptr(), ws.data_ptr(), ws.numel(), dwp.data_ptr(), B, co, ci, kk, ppad, 1, L_in, u,
                  LRELU_SLOPE)
            dub = _floats(dev, co)
            _lib.call('dsv_hgt_bias_grad', dev, Gin.data_ptr(), bws.data_ptr(), bws.numel(), dub.data_ptr(), B, co, L)
            dwv = dwp.view(co, u, kk, ci)                            # tap j of the plain weight sits at phase r_of[j], column t_of[j] (slices: nothing is copied from the host)
            grads[f'ups.{i}.'] = (torch.stack([dwv[:, r_of[j], t_of[j], :] for j in range(k)], 2).permute(1, 0, 2).contiguous(), dub)
            dx = _act(dev, B, ci, L_in)
            _lib.call('dsv_hgt_upsample_dgrad', dev, Gin.data_ptr(), uw.data_ptr(), xup.data_ptr(), dx.data_ptr(), B, ci, co, u, k, L_in, LRELU_SLOPE,
                  float(nk) if i > 0 else 1.0)
            G, L = dx, L_in
        conv_bwd('conv_pre.', G, xin, None, T, 1, 1.0, need_dx=False)
        if nsf:
            H = sines.shape[2]
            dlw, dlb = _floats(dev, H), _floats(dev, 1)
            _lib.call('dsv_hgt_source_backward', dev, dhar.data_ptr(), har.data_ptr(), sines.data_ptr(), dlw.data_ptr(), dlb.data_ptr(), B, Lh, H)
            grads['m_source.l_linear.'] = (dlw.view(1, H), dlb)
        flat = []
        for n, (p, _) in enumerate(layout):
            gw, gb = grads.get(p, (None, None))                      # an NSF generator run without f0: its source and noise_convs are unused
            flat += [gw if ctx.needs_input_grad[5 + 2 * n] else None, gb if ctx.needs_input_grad[6 + 2 * n] else None]
        return (None, None, None, None, None) + tuple(flat)


def hifigan_gen_op(x, f0, rand_ini, noise, h, params, *, return_saved=False):
    """The generator on plain weights (param_layout's order).  return_saved=True: (y, [leaky-ReLU inputs in call order, unpadded], sines or None)."""
    meta = dict(h=h, return_saved=bool(return_saved))
    out = HifiGanGenFunction.apply(x, f0, rand_ini, noise, meta, *params)
    if not return_saved:
        return out
    if f0 is None:
        return out[0], list(out[1:]), None
    return out[0], list(out[1:-1]), out[-1]


def hifigan_generator_losses(gen, mel_loss, x, f0, y, *, lambda_mel, rand_ini=None, noise=None):
    """The mel term of the HiFi-GAN generator objective (configs/tts/hifigan.yaml lambda_mel): y_hat = gen.forward_train(x, f0) on the given
    source draws, mel = mel_loss(y_hat, y) (diffsinger_amd.mel_loss.HifiGanMelLoss; y the recording [B][1][L] or [B][L]), total = lambda_mel * mel.
    The adversarial and the feature-matching terms of the reference's generator objective are NOT part of it: hifigan_training_step adds
    them.  -> (dict(mel, total), y_hat)"""
    y_hat = gen.forward_train(x, f0, rand_ini=rand_ini, noise=noise)
    mel = mel_loss(y_hat, y)
    return {'mel': mel, 'total': lambda_mel * mel}, y_hat


def hifigan_generator_step(gen, mel_loss, batch, hp, opt_g=None):
    """One generator step on the mel term alone, in the shape of pwg_training_step.  batch = dict(x mel [B][80][T], y recording [B][1][T * hop],
    optionally f0 [B][T], rand_ini, noise - the source draws); hp holds lambda_mel and, optionally, generator_grad_norm.  The gradients are zeroed
    here (set_to_none), the objective runs backward, the gradients are clipped ONLY when hp carries generator_grad_norm, opt_g.step() when
    given.  The adversarial and the feature-matching terms are not part of it (see hifigan_generator_losses).
    -> dict(gen_mel, gen_total, gen_grad_norm): the loss terms and the gradient norm before clipping."""
    gparams = [p for p in gen.parameters() if p.requires_grad]
    for p in gparams:
        p.grad = None
    losses, _ = hifigan_generator_losses(gen, mel_loss, batch['x'], batch.get('f0'), batch['y'], lambda_mel=hp['lambda_mel'],
                                         rand_ini=batch.get('rand_ini'), noise=batch.get('noise'))
    losses['total'].backward()
    out = {'gen_' + k: v.detach() for k, v in losses.items()}
    out['gen_grad_norm'] = _clip_and_step(gparams, hp.get('generator_grad_norm'), opt_g)
    return out


def _clip_and_step(params, max_norm, opt):
    """clip_grad_norm_(params, max_norm; None: no clipping) and opt.step() when an optimiser is given -> the norm before clipping.  A
    voc_optim.MultiTensorOptimizer does both itself over ITS parameters, without reading the norm on the host (.grad stays unscaled)."""
    max_norm = float('inf') if max_norm is None else max_norm
    if isinstance(opt, MultiTensorOptimizer):
        return opt.clip_and_step(max_norm)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    if opt is not None:
        opt.step()
    return norm


def hifigan_training_step(gen, discs, mel_loss, batch, hp, opt_g=None, opt_d=None):
    """One step of the HiFi-GAN trainer in the shape of pwg_training_step.  `discs`: a list of modules with MultiPeriodDiscriminator's
    forward(y, y_hat) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs); batch and hp as hifigan_generator_step takes them, hp optionally with
    discriminator_grad_norm; opt_d steps the parameters of every module of `discs`.
    Generator: total = lambda_mel * mel + sum over discs of (adv + fm) (hifigan_generator_losses' parts and hifigan_adversarial_losses), its
    backward, the clip (only when hp carries generator_grad_norm), opt_g's step when given.  Then the discriminators: the gradients the generator's
    terms left on them are dropped, total = sum over discs of (real + fake) of hifigan_discriminator_losses on the detached waveform, its
    backward, the clip at discriminator_grad_norm when given, opt_d's step.  With an empty `discs` the step is hifigan_generator_step.
    -> dict(gen_mel, gen_adv, gen_fm, gen_total, gen_grad_norm, disc_real, disc_fake, disc_total, disc_grad_norm)."""
    from .hifigan_disc import hifigan_adversarial_losses, hifigan_discriminator_losses
    y = batch['y']
    gparams = [p for p in gen.parameters() if p.requires_grad]
    dparams = [p for d in discs for p in d.parameters() if p.requires_grad]
    for p in gparams + dparams:
        p.grad = None
    losses, y_hat = hifigan_generator_losses(gen, mel_loss, batch['x'], batch.get('f0'), y, lambda_mel=hp['lambda_mel'],
                                             rand_ini=batch.get('rand_ini'), noise=batch.get('noise'))
    y3 = y if y.dim() == 3 else y.unsqueeze(1)
    total = losses['total']
    for n, d in enumerate(discs):
        terms = hifigan_adversarial_losses(d, y3, y_hat)
        losses['adv'] = terms['adv'] if n == 0 else losses['adv'] + terms['adv']
        losses['fm'] = terms['fm'] if n == 0 else losses['fm'] + terms['fm']
        total = total + (terms['adv'] + terms['fm'])
    losses['total'] = total
    total.backward()
    out = {'gen_' + k: v.detach() for k, v in losses.items()}
    out['gen_grad_norm'] = _clip_and_step(gparams, hp.get('generator_grad_norm'), opt_g)
    if discs:
        for p in dparams:                                       # the generator's adversarial and feature terms left gradients here
            p.grad = None
        dl = None
        for d in discs:
            real, fake = hifigan_discriminator_losses(d, y3, y_hat)
            dl = {'real': real, 'fake': fake} if dl is None else {'real': dl['real'] + real, 'fake': dl['fake'] + fake}
        dl['total'] = dl['real'] + dl['fake']
        dl['total'].backward()
        out.update({'disc_' + k: v.detach() for k, v in dl.items()})
        out['disc_grad_norm'] = _clip_and_step(dparams, hp.get('discriminator_grad_norm'), opt_d)
    return out
