"""PitchExtractor - mel -> f0 for the NSF vocoder (the reference runs it between the diffusion
sampler and HifiGAN.spec2wav when hparams['pe_enable'], inference/svs/base_svs_infer.py:61-70, tasks/tts/fs2.py:440-445) - as
nn.Modules whose eval forward runs on the HIP operators of libdsdenoise.so (include/dsf.h).

Mirrors the reference module tree (paths relative to the reference root) name for name, so `utils.load_ckpt(pe, hparams['pe_ckpt'],
'model', strict=True)` works on it:

    PitchExtractor, Prenet, ConvStacks, ConvBlock        modules/fastspeech/pe.py:8-148
    ConvNorm                                              modules/commons/common_layers.py:41-59
    PitchPredictor                                        modules/fastspeech/tts_modules.py:192-235 (diffsinger_amd.fs2.PitchPredictor)

What runs where: the seven k = 5 convolutions (+ ReLU), the four Linear layers and the predictor stack are k_fs_conv / k_fs_ln
launches; BatchNorm1d (eval) + the padding mask is k_fs_affine, GroupNorm + ReLU + residual is k_fs_group_norm.  The padding
mask (`mel.abs().sum(-1) == 0`), the positional-embedding lookup and denorm_f0 are torch index ops on the device.  No CPU path.

Training (PitchExtractionTask, tasks/tts/pe.py): in train mode the forward runs under autograd.  BatchNorm1d takes the batch statistics and
updates its running buffers in one launch (dsf_batch_norm_train, Prenet's ReLU and padding mask inside), its backward is one launch;
GroupNorm + ReLU + residual has dsf_group_norm_bwd; the convolutions, LayerNorms and layout changes are the FastSpeech2 training operators
(fs2.py); the predictor's dropout is torch's F.dropout (or, with dropout.enable(), the counter-based HIP op of dropout.py).  pe_losses is the task's loss dict on the fused dsf_f0_loss, pe_training_step the task's
_training_step.  Not covered: synchronising BatchNorm statistics or buffers across ranks (the reference's DDP does not sync the statistics
either), Prenet strides other than 1, ConvBlock norms other than 'gn', a fused dropout."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from .fs2 import Linear, PackedWeight, PitchPredictor, _need_hip, _needs_grad, _stream, conv1d_cm, denorm_f0, from_cm, to_cm
from .hparams import hparams


def channel_affine_cm(x: torch.Tensor, T: int, a: torch.Tensor, b: torch.Tensor, keep=None) -> torch.Tensor:
    _need_hip(x, 'channel_affine')
    lib = _lib.load()
    B, C, TS = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.dsf_channel_affine(x.data_ptr(), a.data_ptr(), b.data_ptr(), keep.data_ptr() if keep is not None else None,
                                          out.data_ptr(), B, C, T, _stream(x.device)), 'dsf_channel_affine')
    return out


def group_norm_cm(x: torch.Tensor, T: int, groups: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, *, relu=False, residual=None):
    _need_hip(x, 'group_norm')
    if _needs_grad(x, gamma, beta, residual):
        return _GroupNormCM.apply(x, gamma, beta, residual, T, int(groups), float(eps), bool(relu))
    return _group_norm_raw(x, T, groups, gamma, beta, eps, relu, residual)


def _group_norm_raw(x, T, groups, gamma, beta, eps, relu, residual):
    lib = _lib.load()
    B, C, TS = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.dsf_group_norm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), residual.data_ptr() if residual is not None else None,
                                      out.data_ptr(), B, C, groups, T, float(eps), int(relu), _stream(x.device)), 'dsf_group_norm')
    return out


class _GroupNormCM(torch.autograd.Function):
    """dsf_group_norm under autograd: dx / dgamma / dbeta by dsf_group_norm_bwd (statistics and ReLU mask recomputed from x); the residual's
    gradient is dy itself."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, T, groups, eps, relu):
        x = x.contiguous()
        res = residual.contiguous() if residual is not None else None
        out = _group_norm_raw(x, T, groups, gamma.detach(), beta.detach(), eps, relu, res)
        ctx.save_for_backward(x, gamma.detach(), beta.detach())
        ctx.cfg = (T, groups, eps, relu, residual is not None)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, beta = ctx.saved_tensors
        T, groups, eps, relu, has_res = ctx.cfg
        B, C, TS = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg = torch.empty(C, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32)
        ws = torch.empty(int(lib.dsf_group_norm_bwd_workspace_floats(B, C)), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(lib.dsf_group_norm_bwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                              ws.data_ptr(), B, C, groups, T, float(eps), int(relu), _stream(x.device)), 'dsf_group_norm_bwd')
        return dx, dg, db, (dy if has_res else None), None, None, None, None


def _batch_norm_train_raw(x, T, gamma, beta, running_mean, running_var, eps, momentum, relu_in, keep):
    lib = _lib.load()
    B, C, TS = x.shape
    out = torch.empty_like(x)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(C, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(lib.dsf_batch_norm_train(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), keep.data_ptr() if keep is not None else None, out.data_ptr(),
                                            mean.data_ptr(), rstd.data_ptr(), running_mean.data_ptr() if running_mean is not None else None,
                                            running_var.data_ptr() if running_var is not None else None, B, C, T, float(eps), float(momentum),
                                            int(relu_in), _stream(x.device)), 'dsf_batch_norm_train')
    return out, mean, rstd


class _BatchNormTrainCM(torch.autograd.Function):
    """dsf_batch_norm_train / dsf_batch_norm_train_bwd.  The running buffers are updated in place by the forward (they are no autograd inputs)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, T, eps, momentum, relu_in, keep):
        x = x.contiguous()
        out, mean, rstd = _batch_norm_train_raw(x, T, gamma.detach(), beta.detach(), running_mean, running_var, eps, momentum, relu_in, keep)
        ctx.save_for_backward(x, gamma.detach(), mean, rstd)
        ctx.keep, ctx.T, ctx.relu_in = keep, T, relu_in
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, mean, rstd = ctx.saved_tensors
        B, C, TS = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg = torch.empty(C, device=x.device, dtype=torch.float32)
        db = torch.empty(C, device=x.device, dtype=torch.float32)
        keep = ctx.keep
        with torch.cuda.device(x.device):
            _lib.check(lib.dsf_batch_norm_train_bwd(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dy.data_ptr(),
                                                    keep.data_ptr() if keep is not None else None, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), B, C,
                                                    ctx.T, int(ctx.relu_in), _stream(x.device)), 'dsf_batch_norm_train_bwd')
        return dx, dg, db, None, None, None, None, None, None, None


def batch_norm_train_cm(x: torch.Tensor, T: int, bn: nn.BatchNorm1d, *, relu_in=False, keep=None) -> torch.Tensor:
    """nn.BatchNorm1d in train mode on a cm tensor: batch statistics over the B * T live columns, y = BN(relu_in ? relu(x) : x) * keep; updates
    bn.running_mean / running_var / num_batches_tracked like the module's own forward."""
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm1d momentum=None (cumulative moving average)')
    if bn.weight is None or bn.bias is None:
        raise NotImplementedError('BatchNorm1d affine=False')
    _need_hip(x, 'batch_norm_train')
    rm, rv = (bn.running_mean, bn.running_var) if bn.track_running_stats else (None, None)
    if _needs_grad(x, bn.weight, bn.bias):
        out = _BatchNormTrainCM.apply(x, bn.weight, bn.bias, rm, rv, T, float(bn.eps), float(bn.momentum), bool(relu_in), keep)
    else:
        out = _batch_norm_train_raw(x.contiguous(), T, bn.weight.detach(), bn.bias.detach(), rm, rv, bn.eps, bn.momentum, relu_in, keep)[0]
    if bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return out


class Prenet(nn.Module):
    """pe.py:8-41 (strides 1).  forward_cm: channel-major mel -> channel-major hidden (the module's second return value)."""

    def __init__(self, in_dim=80, out_dim=256, kernel=5, n_layers=3, strides=None):
        super().__init__()
        if strides is not None and any(s != 1 for s in strides):
            raise NotImplementedError('Prenet strides other than 1')
        self.kernel = kernel
        layers = []
        for _ in range(n_layers):
            layers.append(nn.Sequential(nn.Conv1d(in_dim, out_dim, kernel_size=kernel, padding=kernel // 2), nn.ReLU(), nn.BatchNorm1d(out_dim)))
            in_dim = out_dim
        self.layers = nn.ModuleList(layers)
        self.out_proj = nn.Linear(out_dim, out_dim)
        self._packs = [PackedWeight() for _ in range(n_layers)]
        self._pout = PackedWeight()

    def forward(self, x):
        """x [B,T,80] -> (hiddens [1,B,T,H], out [B,T,H]) like the reference module (pe.py:23-41)."""
        keep = (~x.abs().sum(-1).eq(0)).float().contiguous()
        T = x.shape[1]
        h, out = self.forward_cm(to_cm(x), T, keep, return_hidden=True)
        return from_cm(h, T)[None], from_cm(out, T)

    def forward_cm(self, x, T, keep, return_hidden=False):
        for seq, pk in zip(self.layers, self._packs):
            conv, bn = seq[0], seq[2]
            if bn.training:                                          # batch statistics; the ReLU and the padding mask are inside the launch
                y = conv1d_cm(x, T, conv.weight, pk, conv.bias)
                x = batch_norm_train_cm(y, T, bn, relu_in=True, keep=keep)
                continue
            y = conv1d_cm(x, T, conv.weight, pk, conv.bias, act='relu')
            inv = 1.0 / torch.sqrt(bn.running_var + bn.eps)          # aten batch_norm_cpu_transform_input: alpha = invstd * weight,
            a = (inv * bn.weight).contiguous()                       # beta = bias - mean * alpha, out = x * alpha + beta
            b = (bn.bias - bn.running_mean * a).contiguous()
            x = channel_affine_cm(y, T, a, b, keep)
        out = conv1d_cm(x, T, self.out_proj.weight, self._pout, self.out_proj.bias, keep=keep)
        return (x, out) if return_hidden else out


class ConvNorm(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1):
        super().__init__()
        assert kernel_size % 2 == 1
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, padding=(kernel_size - 1) // 2)
        nn.init.xavier_uniform_(self.conv.weight, gain=nn.init.calculate_gain('linear'))


class ConvBlock(nn.Module):
    """pe.py:44-79 with norm 'gn' (the only one PitchExtractor builds)."""

    def __init__(self, idim=80, n_chans=256, kernel_size=3, norm='gn'):
        super().__init__()
        if norm != 'gn':
            raise NotImplementedError(f"ConvBlock norm {norm!r}")
        self.conv = ConvNorm(idim, n_chans, kernel_size)
        self.norm = nn.GroupNorm(n_chans // 16, n_chans)
        self._pack = PackedWeight()


class ConvStacks(nn.Module):
    """pe.py:82-116, res=True, strides 1."""

    def __init__(self, idim=80, n_layers=5, n_chans=256, odim=32, kernel_size=5, norm='gn'):
        super().__init__()
        self.kernel_size = kernel_size
        self.in_proj = Linear(idim, n_chans)
        self.conv = nn.ModuleList([ConvBlock(n_chans, n_chans, kernel_size, norm=norm) for _ in range(n_layers)])
        self.out_proj = Linear(n_chans, odim)
        self._pin, self._pout = PackedWeight(), PackedWeight()

    def forward_cm(self, x, T):
        x = conv1d_cm(x, T, self.in_proj.weight, self._pin, self.in_proj.bias)
        for blk in self.conv:
            c = blk.conv.conv
            y = conv1d_cm(x, T, c.weight, blk._pack, c.bias)
            x = group_norm_cm(y, T, blk.norm.num_groups, blk.norm.weight, blk.norm.bias, blk.norm.eps, relu=True, residual=x)
        return conv1d_cm(x, T, self.out_proj.weight, self._pout, self.out_proj.bias)


class PitchExtractor(nn.Module):
    """pe.py:119-148.  forward(mel [B,T,80]) -> {'pitch_pred' [B,T,2], 'f0_denorm_pred' [B,T]}."""

    def __init__(self, n_mel_bins=80, conv_layers=2):
        super().__init__()
        self.hidden_size = hparams['hidden_size']
        self.predictor_hidden = hparams['predictor_hidden'] if hparams['predictor_hidden'] > 0 else self.hidden_size
        self.conv_layers = conv_layers
        self.mel_prenet = Prenet(n_mel_bins, self.hidden_size, strides=[1, 1, 1])
        if conv_layers > 0:
            self.mel_encoder = ConvStacks(idim=self.hidden_size, n_chans=self.hidden_size, odim=self.hidden_size, n_layers=conv_layers)
        self.pitch_predictor = PitchPredictor(self.hidden_size, n_chans=self.predictor_hidden, n_layers=5, dropout_rate=0.1, odim=2,
                                              padding=hparams['ffn_padding'], kernel_size=hparams['predictor_kernel'])

    def forward(self, mel_input=None):
        """Train mode runs under autograd (batch statistics in Prenet's BatchNorm1d, dropout in the predictor); eval mode under no_grad."""
        _need_hip(mel_input, 'PitchExtractor')
        if self.training:
            return self._forward(mel_input)
        with torch.no_grad():
            return self._forward(mel_input)

    def _forward(self, mel_input):
        mel_input = mel_input.to(torch.float32)
        B, T, _ = mel_input.shape
        pitch_padding = mel_input.abs().sum(-1) == 0
        keep = (~pitch_padding).float().contiguous()
        x = self.mel_prenet.forward_cm(to_cm(mel_input), T, keep)
        if self.conv_layers > 0:
            x = self.mel_encoder.forward_cm(x, T)
        ret = {}
        ret['pitch_pred'] = pitch_pred = self.pitch_predictor(from_cm(x, T))
        use_uv = hparams['pitch_type'] == 'frame' and hparams['use_uv']
        ret['f0_denorm_pred'] = denorm_f0(pitch_pred[:, :, 0].clone(), (pitch_pred[:, :, 1] > 0) if use_uv else None, hparams,
                                          pitch_padding=pitch_padding)
        return ret


class _F0Loss(torch.autograd.Function):
    """out = [uv, f0, sum nonpadding, sum nonpadding'] of add_f0_loss; dsf_f0_loss / dsf_f0_loss_bwd."""

    @staticmethod
    def forward(ctx, pred, f0, uv, nonpadding, use_uv, l2, lam_uv, lam_f0):
        lib = _lib.load()
        B, T, Cp = pred.shape
        ws = torch.empty(int(lib.dsf_f0_loss_workspace_floats()), device=pred.device, dtype=torch.float32)
        out = torch.empty(4, device=pred.device, dtype=torch.float32)
        _lib.call('dsf_f0_loss', pred.device, pred.data_ptr(), pred.stride(0), pred.stride(1), pred.stride(2), f0.data_ptr(),
                  _lib.ptr(uv if use_uv else None), nonpadding.data_ptr(), B, T, Cp, int(use_uv), int(l2), float(lam_uv), float(lam_f0), ws.data_ptr(),
                  out.data_ptr())
        ctx.save_for_backward(pred, f0, uv if use_uv else f0, nonpadding, out)
        ctx.cfg = (bool(use_uv), bool(l2), float(lam_uv), float(lam_f0))
        return out

    @staticmethod
    def backward(ctx, g):
        pred, f0, uv, nonpadding, out = ctx.saved_tensors
        use_uv, l2, lam_uv, lam_f0 = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        B, T, Cp = pred.shape
        g2 = g[:2].contiguous()
        dp = torch.empty((B, T, Cp), device=pred.device, dtype=torch.float32)
        _lib.call('dsf_f0_loss_bwd', pred.device, pred.data_ptr(), pred.stride(0), pred.stride(1), pred.stride(2), f0.data_ptr(),
                  _lib.ptr(uv if use_uv else None), nonpadding.data_ptr(), B, T, Cp, int(use_uv), int(l2), lam_uv, lam_f0, out.data_ptr(), g2.data_ptr(),
                  dp.data_ptr())
        return dp, None, None, None, None, None, None, None


def _f32_bt(name, t, shape, dev):
    if not torch.is_tensor(t) or t.device != dev:
        raise ValueError(f'{name}: a tensor on {dev} is required (there is no CPU path)')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: shape {tuple(shape)} required, got {tuple(t.shape)}')
    return t.detach().to(torch.float32).contiguous()


def f0_loss_terms(pitch_pred, f0, uv, nonpadding, *, use_uv=True, pitch_loss='l1', lam_uv=1.0, lam_f0=1.0):
    """FastSpeech2Task.add_f0_loss (tasks/tts/fs2.py:254-269) as one fused operator: a [4] tensor (uv loss, f0 loss, sum nonpadding, sum of
    nonpadding * (uv == 0)).  pitch_pred [B,T,>=1 (2 with use_uv)] fp32 with any strides; f0 / uv / nonpadding [B,T]."""
    _need_hip(pitch_pred, 'f0_loss')
    if pitch_loss not in ('l1', 'l2'):
        raise NotImplementedError(f'pitch_loss {pitch_loss!r}')
    if pitch_pred.dim() != 3 or pitch_pred.dtype != torch.float32 or pitch_pred.shape[2] < (2 if use_uv else 1):
        raise ValueError(f'pitch_pred: fp32 [B, T, {2 if use_uv else 1}+] required, got {pitch_pred.dtype} {tuple(pitch_pred.shape)}')
    bt, dev = pitch_pred.shape[:2], pitch_pred.device
    f0 = _f32_bt('f0', f0, bt, dev)
    uv = _f32_bt('uv', uv, bt, dev) if use_uv else None
    nonpadding = _f32_bt('nonpadding', nonpadding, bt, dev)
    return _F0Loss.apply(pitch_pred, f0, uv, nonpadding, bool(use_uv), pitch_loss == 'l2', float(lam_uv), float(lam_f0))


def pe_losses(output: dict, sample: dict, hp: dict) -> dict:
    """The loss dict of PitchExtractionTask.run_model (tasks/tts/pe.py:128-155): {'uv' (use_uv), 'f0'}, the reference's keys, order and lambdas."""
    if hp['pitch_loss'] == 'ssim':
        raise NotImplementedError("pitch_loss 'ssim': the reference computes no f0 loss for it (tasks/tts/fs2.py:268-269)")
    nonpadding = (sample['mels'].abs().sum(-1) > 0).float()
    use_uv = bool(hp['use_uv'])
    t = f0_loss_terms(output['pitch_pred'], sample['f0'], sample['uv'] if use_uv else None, nonpadding, use_uv=use_uv, pitch_loss=hp['pitch_loss'],
                      lam_uv=hp['lambda_uv'] if use_uv else 0.0, lam_f0=hp['lambda_f0'])
    losses = {}
    if use_uv:
        losses['uv'] = t[0]
    losses['f0'] = t[1]
    return losses


def pe_training_step(model, sample: dict, hp: dict):
    """PitchExtractionTask._training_step (tasks/tts/pe.py:111-115): (total_loss, loss_dict); loss_dict carries 'batch_size'."""
    losses = pe_losses(model(sample['mels']), sample, hp)
    total = sum(v for v in losses.values() if isinstance(v, torch.Tensor) and v.requires_grad)
    losses['batch_size'] = sample['mels'].size()[0]
    return total, losses
