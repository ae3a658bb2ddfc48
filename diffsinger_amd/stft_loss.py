"""The multi-resolution STFT loss on the device - the operators of include/dsv.h, section "STFT loss" (kernels: csrc/voc_stft_loss.hpp), on torch
device tensors, and the reference's criterion built on them (modules/parallel_wavegan/losses/stft_loss.py, again in
modules/parallel_wavegan/stft_loss.py; configured by configs/tts/pwg.yaml:77-82).

    stft_adjoint_op          the vector-Jacobian product of stft_op (what autograd calls when a waveform passed to stft_op requires grad)
    spectral_loss_op         (sc, mag) of two spectra: stft_loss.py:26-31, :52, :73; gradient with respect to the first
    STFTLoss, MultiResolutionSTFTLoss      stft_loss.py:76-153 with the reference's constructor signatures and defaults

The reference's module cannot run on torch 2.x (it calls torch.stft without return_complex); what it computes there is torch.stft's default
framing: centred, reflect padding of n_fft / 2, periodic Hann window of win_length centred in the frame - stft_op(center=True,
pad_mode='reflect'), the entry point the loss calls.

torch is plumbing (buffers, streams, the autograd graph).  There is no CPU path.  Nothing here synchronises or reads a device value on the
host: after one warm-up call (which builds the bases) the whole forward and backward records into one torch.cuda.graph."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import stft as ST

__all__ = ['stft_adjoint_op', 'spectral_loss_op', 'STFTLoss', 'MultiResolutionSTFTLoss']


def _adjoint_launch(g, L, n_fft, hop, win_length, pl, pr, pad_mode):
    """dsv_stft_adjoint on validated arguments: g float32 [B][n_bins][n_frames][2] contiguous -> [B][L]"""
    B, _, T, _ = g.shape
    adj = ST.adjoint_basis(g.device, n_fft, win_length)
    lib = _lib.load()
    ws = torch.empty(lib.dsv_stft_adjoint_workspace_floats(B, T, n_fft), device=g.device, dtype=torch.float32)
    dx = torch.empty(B, L, device=g.device, dtype=torch.float32)
    with torch.cuda.device(g.device):
        _lib.check(lib.dsv_stft_adjoint(g.data_ptr(), adj.data_ptr(), ws.data_ptr(), dx.data_ptr(), B, L, n_fft, hop, pl, pr,
                                        ST._PAD_MODES[pad_mode], ST._stream(g.device)), 'dsv_stft_adjoint')
    return dx


class StftFunction(torch.autograd.Function):
    """stft_op with a gradient: forward dsv_stft, backward dsv_stft_adjoint.  x float32 [B][L] -> float32 [B][n_bins][n_frames][2]."""

    @staticmethod
    def forward(ctx, x, n_fft, hop, win_length, pl, pr, pad_mode, fc):
        ST.adjoint_basis(x.device, n_fft, win_length)          # here, not in backward: a warm-up FORWARD is then enough before a capture
        ctx.geometry = (x.shape[1], n_fft, hop, win_length, pl, pr, pad_mode)
        return ST._stft_launch(x, None, n_fft, hop, win_length, pl, pr, pad_mode, None, fc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (_adjoint_launch(g.to(torch.float32).contiguous(), *ctx.geometry),) + (None,) * 7


def _real_view(S, n_bins, what):
    """complex [B][n_bins][T] (or [n_bins][T]) or float [B][n_bins][T][2] -> (float32 view [B][n_bins][T][2], was complex)"""
    if not isinstance(S, torch.Tensor):
        raise ValueError(f'{what}: needs a tensor')
    cplx = S.is_complex()
    if cplx:
        if S.dim() == 2:
            S = S[None]
        S = torch.view_as_real(S.to(torch.complex64).contiguous())
    if S.dim() != 4 or S.shape[3] != 2 or (n_bins is not None and S.shape[1] != n_bins) or min(S.shape) < 1:
        bins = 'n_bins' if n_bins is None else n_bins
        raise ValueError(f'{what}: spectrum must be complex [B][{bins}][n_frames] or float [B][{bins}][n_frames][2], got {tuple(S.shape)}')
    return S.to(torch.float32).contiguous(), cplx


def stft_adjoint_op(G, length, *, n_fft, hop, win_length=None, center=True, pad_mode='constant', pad=None):
    """The transpose of stft_op(wav [B][length], same arguments): cotangent G, complex64 [B][n_fft / 2 + 1][n_frames] (torch's convention:
    dL/dre + i dL/dim) or float [B][n_bins][n_frames][2], -> dL/dwav [B][length].  Frame gradients by the MFMA product of istft_op against the
    transposed forward basis (analysis window, no 1 / n_fft, no factor 2; the imaginary cotangents of bin 0 and bin n_fft / 2 are ignored),
    then a gather in ascending frame order with the padding folded back: zero padding drops, reflect padding adds the mirrors' sums."""
    win_length = n_fft if win_length is None else win_length
    ST._check_geometry(n_fft, hop, win_length)
    if pad_mode not in ST._PAD_MODES:
        raise ValueError(f"pad_mode={pad_mode!r}: 'constant' or 'reflect'")
    g, _ = _real_view(G, n_fft // 2 + 1, 'stft_adjoint_op')
    L = int(length)
    if L < 1:
        raise ValueError(f'stft_adjoint_op: length={length} must be >= 1')
    pl, pr = ST._pads(n_fft, center, pad)
    if pad_mode == 'reflect' and max(pl, pr) >= L:
        raise ValueError(f'reflect padding ({pl}, {pr}) must be smaller than the signal (L={L})')
    T = ST.n_frames(L, n_fft, hop, pl, pr)
    if g.shape[2] != T or not 1 <= g.shape[0] <= 65535:
        raise ValueError(f'stft_adjoint_op: a waveform of {L} samples has {T} frames, the cotangent {g.shape[2]} (B={g.shape[0]} in [1, 65535])')
    if not g.is_cuda:
        raise RuntimeError('stft_adjoint_op: needs a device tensor (there is no CPU path)')
    return _adjoint_launch(g, L, n_fft, hop, win_length, pl, pr, pad_mode)


class SpectralLossFunction(torch.autograd.Function):
    """X, Y float32 [..][2] contiguous -> out [2] = (sc, mag); gradient with respect to X."""

    @staticmethod
    def forward(ctx, X, Y):
        lib = _lib.load()
        n = X.numel() // 2
        ws = torch.empty(lib.dsv_spectral_loss_workspace_floats(n) // 2, device=X.device, dtype=torch.float64)
        out = torch.empty(2, device=X.device, dtype=torch.float32)
        with torch.cuda.device(X.device):
            _lib.check(lib.dsv_spectral_loss(X.data_ptr(), Y.data_ptr(), ws.data_ptr(), out.data_ptr(), n, ST._stream(X.device)), 'dsv_spectral_loss')
        ctx.save_for_backward(X, Y, ws)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        X, Y, ws = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        G = torch.empty_like(X)
        with torch.cuda.device(X.device):
            _lib.check(_lib.load().dsv_spectral_loss_backward(X.data_ptr(), Y.data_ptr(), ws.data_ptr(), g.data_ptr(), G.data_ptr(), X.numel() // 2,
                                                              ST._stream(X.device)), 'dsv_spectral_loss_backward')
        return G, None


def spectral_loss_op(X, Y):
    """Spectra X (prediction), Y (target), both complex [B][n_bins][n_frames] or both float [B][n_bins][n_frames][2], -> float32 [2]:
        sc  = ||ym - xm||_F / ||ym||_F,   mag = mean |ln ym - ln xm|,   m = sqrt(max(re^2 + im^2, 1e-7))
    over the whole block.  The gradient flows to X only (exactly 0 where X's clamp is active); a target that requires grad raises
    NotImplementedError."""
    Xr, cx = _real_view(X, None, 'spectral_loss_op')
    Yr, cy = _real_view(Y, None, 'spectral_loss_op')
    if cx != cy or Xr.shape != Yr.shape:
        raise ValueError(f'spectral_loss_op: the spectra must share layout and shape, got {tuple(X.shape)} {X.dtype} and {tuple(Y.shape)} {Y.dtype}')
    if Xr.device != Yr.device:
        raise ValueError(f'spectral_loss_op: the spectra are on different devices ({Xr.device}, {Yr.device})')
    if Y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('spectral_loss_op: no gradient with respect to the target spectrum (detach it)')
    if not Xr.is_cuda:
        raise NotImplementedError('spectral_loss_op: needs device tensors (there is no CPU path)')
    return SpectralLossFunction.apply(Xr, Yr)


def _check_resolution(fft_size, shift_size, win_length, window, use_mel_loss):
    if window != 'hann_window':
        raise NotImplementedError(f"window={window!r}: the STFT bases carry the periodic Hann window only ('hann_window')")
    if use_mel_loss:
        raise NotImplementedError('use_mel_loss=True is not supported (the reference needs librosa.filters.mel for it)')
    ST._check_geometry(fft_size, shift_size, win_length)


def _check_pair(x, y, fft_sizes, who):
    """Everything forward refuses, before any launch - and before the device is asked for, so that it holds on a host without one."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise ValueError(f'{who}: x and y must be tensors')
    if x.dim() != 2 or x.shape != y.shape or x.shape[0] < 1 or x.shape[0] > 65535:
        raise ValueError(f'{who}: x and y must both be [B][T] with 1 <= B <= 65535, got {tuple(x.shape)} and {tuple(y.shape)}')
    if not x.is_floating_point() or not y.is_floating_point():
        raise ValueError(f'{who}: x and y must be floating-point waveforms, got {x.dtype} and {y.dtype}')
    if x.device != y.device:
        raise ValueError(f'{who}: x and y are on different devices ({x.device}, {y.device})')
    T = x.shape[1]
    for n_fft in fft_sizes:
        if T <= n_fft // 2:
            raise ValueError(f'{who}: reflect padding of n_fft / 2 = {n_fft // 2} needs T > {n_fft // 2} samples, got T={T}')
    if y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f'{who}: no gradient with respect to the target waveform y (detach it)')
    if not x.is_cuda:
        raise NotImplementedError(f'{who}: needs device tensors (there is no CPU path)')


def _resolution_loss(x, y, n_fft, hop, win):
    X = ST.stft_op(x, n_fft=n_fft, hop=hop, win_length=win, center=True, pad_mode='reflect')
    with torch.no_grad():
        Y = ST.stft_op(y, n_fft=n_fft, hop=hop, win_length=win, center=True, pad_mode='reflect')
    return spectral_loss_op(X, Y)


class STFTLoss(torch.nn.Module):
    """stft_loss.py:76-106: forward(x, y), x the predicted and y the recorded waveform [B][T], -> (sc_loss, mag_loss), 0-dim tensors."""

    def __init__(self, fft_size=1024, shift_size=120, win_length=600, window='hann_window', use_mel_loss=False):
        super().__init__()
        _check_resolution(fft_size, shift_size, win_length, window, use_mel_loss)
        self.fft_size, self.shift_size, self.win_length = int(fft_size), int(shift_size), int(win_length)

    def forward(self, x, y):
        _check_pair(x, y, (self.fft_size,), 'STFTLoss')
        out = _resolution_loss(x, y, self.fft_size, self.shift_size, self.win_length)
        return out[0], out[1]


class MultiResolutionSTFTLoss(torch.nn.Module):
    """stft_loss.py:109-153: the mean of (sc, mag) over the resolutions, added in the order given."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), window='hann_window', use_mel_loss=False):
        super().__init__()
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)) or len(fft_sizes) < 1:
            raise ValueError(f'fft_sizes, hop_sizes and win_lengths must have one entry per resolution, got {len(fft_sizes)}, {len(hop_sizes)}, {len(win_lengths)}')
        self.stft_losses = torch.nn.ModuleList(STFTLoss(fs, ss, wl, window, use_mel_loss) for fs, ss, wl in zip(fft_sizes, hop_sizes, win_lengths))

    def forward(self, x, y):
        _check_pair(x, y, [f.fft_size for f in self.stft_losses], 'MultiResolutionSTFTLoss')
        total = None
        for f in self.stft_losses:
            out = _resolution_loss(x, y, f.fft_size, f.shift_size, f.win_length)
            total = out if total is None else total + out
        total = total / len(self.stft_losses)
        return total[0], total[1]
