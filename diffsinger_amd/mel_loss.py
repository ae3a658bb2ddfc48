"""The mel-spectrogram loss of the HiFi-GAN trainer on the device: the L1 distance between the log-mel of the generated waveform and the
recording's (modules/hifigan/mel_utils.py:45-76 behind configs/tts/hifigan.yaml `lambda_mel: 45.0`), the generator's dominant objective.

    mel_spectrogram_loss_op      mean |logmel(wav) - target| from a waveform and a ready log-mel
    HifiGanMelLoss(hparams)      the criterion as a module: forward(y_hat, y) or forward(y_hat, mel=...)

Composed from operators that exist: the differentiable log-mel of diffsinger_amd.stft.logmel_op (include/dsv.h, section "Mel loss": spectrum ->
head, and back head backward -> adjoint STFT -> clamp mask) and the deterministic L1 mean of the FastSpeech2 losses (dsf_l1_mean / dsf_l1_mean_bwd,
include/dsf.h).  Launches of one loss forward + backward with a waveform target: 2 (prediction) + 2 (target) + 2 (L1 mean) forward, 1 (L1) + 1
(head) + 2 (adjoint) + 1 (clamp mask) backward.

The reference's mel_spectrogram cannot run on torch 2.x (torch.stft without return_complex) and takes its basis from librosa; the basis here is
data of the caller (diffsinger_amd.stft.mel_filterbank restates librosa's default).

torch is plumbing (buffers, streams, the autograd graph).  There is no CPU path.  Nothing here synchronises or reads a device value on the
host: after one warm-up call (which builds the bases) forward and backward record into one torch.cuda.graph."""
from __future__ import annotations

import torch

from . import stft as ST

__all__ = ['mel_spectrogram_loss_op', 'HifiGanMelLoss']

_HPARAM_KEYS = ('fft_size', 'hop_size', 'win_size', 'audio_num_mel_bins', 'fmin', 'fmax', 'audio_sample_rate')


def _wave_rows(w, who, name):
    """[B][L] or [B][1][L] -> [B][L]"""
    if not isinstance(w, torch.Tensor) or not w.is_floating_point():
        raise ValueError(f'{who}: {name} must be a floating-point tensor')
    if w.dim() == 3 and w.shape[1] == 1:
        w = w[:, 0]
    if w.dim() != 2 or not 1 <= w.shape[0] <= 65535 or w.shape[1] < 1:
        raise ValueError(f'{who}: {name} must be [B][L] or [B][1][L] with 1 <= B <= 65535, got {tuple(w.shape)}')
    return w


def _check_basis(mel_basis, n_fft, who):
    if not isinstance(mel_basis, torch.Tensor) or mel_basis.dim() != 2 or mel_basis.shape[1] != n_fft // 2 + 1:
        raise ValueError(f'{who}: mel_basis must be a tensor [M][{n_fft // 2 + 1}]')
    if not 1 <= mel_basis.shape[0] <= ST.MAX_MEL_BINS:
        raise ValueError(f'{who}: M={mel_basis.shape[0]} mel bins: at most {ST.MAX_MEL_BINS} are supported')
    if mel_basis.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f'{who}: no gradient with respect to the mel basis (detach it)')


def _l1_mean(target, pred):
    from .train import _L1Mean
    return _L1Mean.apply(target, pred)


def mel_spectrogram_loss_op(wav, target_logmel, mel_basis, *, n_fft, hop, win_length=None, flavour='hifigan'):
    """mean |logmel_op(wav, mel_basis, flavour) - target_logmel| over all B * T * M cells, a 0-dim tensor: wav [B][L] (or [B][1][L]),
    target_logmel [B][T][M] with T the frame count of L samples, mel_basis [M][n_fft / 2 + 1].  The gradient flows to `wav` only (the L1's
    sign(0) is 0; the log-mel's gradient is exactly 0 at floored cells and behind clamped samples); a target or a basis that requires grad
    raises NotImplementedError.  Sums in a fixed order: two calls are bitwise equal."""
    who = 'mel_spectrogram_loss_op'
    win_length = n_fft if win_length is None else win_length
    ST._check_geometry(n_fft, hop, win_length)
    x = _wave_rows(wav, who, 'wav')
    _check_basis(mel_basis, n_fft, who)
    if not isinstance(target_logmel, torch.Tensor) or target_logmel.dim() != 3 or target_logmel.shape[0] != x.shape[0] \
            or target_logmel.shape[2] != mel_basis.shape[0]:
        raise ValueError(f'{who}: target_logmel must be [B={x.shape[0]}][T][M={mel_basis.shape[0]}], got '
                         f'{tuple(target_logmel.shape) if isinstance(target_logmel, torch.Tensor) else type(target_logmel)}')
    if target_logmel.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f'{who}: no gradient with respect to the target (detach it)')
    if not x.is_cuda or not target_logmel.is_cuda or not mel_basis.is_cuda:
        raise RuntimeError(f'{who}: needs device tensors (there is no CPU path)')
    pred = ST.logmel_op(x, mel_basis, n_fft=n_fft, hop=hop, win_length=win_length, flavour=flavour)
    if pred.shape != target_logmel.shape:
        raise ValueError(f'{who}: a waveform of {x.shape[1]} samples has {pred.shape[1]} frames, the target {target_logmel.shape[1]}')
    tgt = target_logmel.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    return _l1_mean(tgt, pred)


class HifiGanMelLoss(torch.nn.Module):
    """The mel term of the HiFi-GAN generator objective.  hparams: fft_size, hop_size, win_size, audio_num_mel_bins, fmin, fmax (-1: 0 /
    Nyquist), audio_sample_rate; the basis is diffsinger_amd.stft.mel_basis_on(...) of them unless `mel_basis` [M][fft_size / 2 + 1] gives the
    caller's own data (librosa.filters.mel(...) for the reference's numbers).
    forward(y_hat, y) / forward(y_hat, mel=target_logmel): y_hat the generated and y the recorded waveform, [B][L] or [B][1][L]; a waveform
    target is analysed without grad through the SAME two launches as the prediction (so loss(x, x) is exactly 0), a ready log-mel
    [B][T][M] is taken as it is.  -> 0-dim mean |logmel(y_hat) - target|."""

    def __init__(self, hparams, mel_basis=None):
        super().__init__()
        missing = [k for k in _HPARAM_KEYS if k not in hparams or hparams[k] is None]
        if missing:
            raise KeyError(f'HifiGanMelLoss: hparams lack {missing} (needed: {list(_HPARAM_KEYS)})')
        self.n_fft, self.hop, self.win = int(hparams['fft_size']), int(hparams['hop_size']), int(hparams['win_size'])
        ST._check_geometry(self.n_fft, self.hop, self.win)
        self.M, self.sr = int(hparams['audio_num_mel_bins']), hparams['audio_sample_rate']
        if not 1 <= self.M <= ST.MAX_MEL_BINS:
            raise ValueError(f'HifiGanMelLoss: M={self.M} mel bins: at most {ST.MAX_MEL_BINS} are supported')
        fmin, fmax = hparams['fmin'], hparams['fmax']
        self.fmin, self.fmax = (0 if fmin == -1 else fmin), (self.sr / 2 if fmax == -1 else fmax)
        if mel_basis is not None:
            _check_basis(mel_basis, self.n_fft, 'HifiGanMelLoss')
            if mel_basis.shape[0] != self.M:
                raise ValueError(f'HifiGanMelLoss: mel_basis has {mel_basis.shape[0]} rows, audio_num_mel_bins is {self.M}')
            self.register_buffer('mel_basis', mel_basis.detach().to(torch.float32).clone(), persistent=False)
        else:
            self.mel_basis = None

    def basis_on(self, device):
        if self.mel_basis is not None:
            return self.mel_basis
        return ST.mel_basis_on(device, self.sr, self.n_fft, self.M, self.fmin, self.fmax)

    def analyse(self, wav):
        """The target path: the log-mel [B][T][M] of a waveform through spectrum -> head, without grad."""
        x = _wave_rows(wav, 'HifiGanMelLoss', 'y')
        with torch.no_grad():
            return ST.LogmelFunction.apply(*self._chain_args(x))

    def _chain_args(self, x):
        o = ST._FLAVOURS['hifigan']
        x = ST._rows(x, 'HifiGanMelLoss')
        pad = (self.n_fft - self.hop) // 2
        if pad >= x.shape[1]:
            raise ValueError(f'reflect padding ({pad}, {pad}) must be smaller than the signal (L={x.shape[1]})')
        ST.n_frames(x.shape[1], self.n_fft, self.hop, pad, pad)
        mb = self.basis_on(x.device).to(device=x.device, dtype=torch.float32).contiguous()
        return (x, mb, self.n_fft, self.hop, self.win, pad, pad, o['pad_mode'], bool(o['clamp']), float(o['mag_eps']), float(o['floor']),
                bool(o['log10']))

    def forward(self, y_hat, y=None, *, mel=None):
        who = 'HifiGanMelLoss'
        if (y is None) == (mel is None):
            raise ValueError(f'{who}: give the target as a waveform y or as a log-mel mel=, not both')
        x = _wave_rows(y_hat, who, 'y_hat')
        tgt = y if mel is None else mel
        if not isinstance(tgt, torch.Tensor):
            raise ValueError(f'{who}: the target must be a tensor')
        if tgt.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f'{who}: no gradient with respect to the target (detach it)')
        if mel is None:
            yr = _wave_rows(y, who, 'y')
            if yr.shape != x.shape:
                raise ValueError(f'{who}: y_hat and y must have one shape, got {tuple(x.shape)} and {tuple(yr.shape)}')
        elif mel.dim() != 3 or mel.shape[0] != x.shape[0] or mel.shape[2] != self.M:
            raise ValueError(f'{who}: mel= must be [B={x.shape[0]}][T][M={self.M}], got {tuple(mel.shape)}')
        if not x.is_cuda or not tgt.is_cuda:
            raise RuntimeError(f'{who}: needs device tensors (there is no CPU path)')
        args = self._chain_args(x)
        if mel is None:
            tgt = self.analyse(y)
        else:
            tgt = mel.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if x.requires_grad and torch.is_grad_enabled():
            pred = ST.LogmelFunction.apply(*args)
        else:
            with torch.no_grad():
                pred = ST.LogmelFunction.apply(*args)
        if pred.shape != tgt.shape:
            raise ValueError(f'{who}: a waveform of {x.shape[1]} samples has {pred.shape[1]} frames, the target {tgt.shape[1]}')
        return _l1_mean(tgt, pred)
