"""Test infrastructure of the mel loss (include/dsv.h, section "Mel loss"): float64 restatements on the CPU built ONLY from torch, numpy and
tests/stft_helpers / tests/stft_loss_helpers - never from diffsinger_amd (its mel_filterbank is used as DATA by the callers) - with the float32
yardsticks the GPU bounds come from.

    head64 / head32              spectrum [B][n_bins][T][2] -> (log-mel, linear mel) [B][T][M]: sqrt(re^2 + im^2 + mag_eps), W @ ., log(max(., floor))
    head_vjp64 / head_vjp32      the vector-Jacobian product of the head as the formula of csrc/voc_mel.hpp; the floor branch is decided on a
                                 SUPPLIED linear mel (the tests pass the device's saved one: a float32 rounding of a cell that sits on the
                                 floor then cannot turn into a gradient jump, and no cell needs to be left out)
    stft_vjp                     the transpose of the framing of a flavour (any padding amount) from tests.stft_loss_helpers.vjp64 (float64,
                                 autograd) / .adjoint_matmul (float32, the family's yardstick) on the padded length, the padding folded by autograd
    clamp_mask                   1 where -1 <= x <= 1 (torch.clamp's gradient mask), for flavours that clamp
    ref_loss64                   the loss from waveforms through tests.stft_helpers.ref_logmel64
    signals                      the inputs of the GPU tests

The yardstick rule of the family: the kernel and the float32 CPU evaluation are fp32 sums of the same products in a different order; the GPU bound
is 2 x the float32 evaluation's error against float64, both from the same (the device's own) operands."""
import numpy as np
import torch

from tests import stft_helpers as SH
from tests import stft_loss_helpers as LH

GEOMETRIES = ((1024, 256, 1024, 22050, 80, 80, 7600), (512, 128, 512, 24000, 80, 30, 12000), (2048, 512, 2048, 44100, 128, 40, 16000),
              (256, 64, 256, 16000, 40, 0, 8000))                       # (n_fft, hop, win, sr, M, fmin, fmax)


def f32(v):
    """a parameter as the C ABI receives it"""
    return float(np.float32(v))


def _head(S, W, mag_eps, floor, log10, dt):
    S, W = torch.as_tensor(S).to(dt), torch.as_tensor(W).to(dt)
    re, im = S[..., 0], S[..., 1]
    mag = torch.sqrt(re * re + im * im + torch.tensor(f32(mag_eps), dtype=dt))        # [B][n_bins][T]
    mel = torch.matmul(W, mag)                                                        # [B][M][T]
    clipped = torch.clamp(mel, min=f32(floor))
    out = torch.log10(clipped) if log10 else torch.log(clipped)
    return out.transpose(1, 2), mel.transpose(1, 2)


def head64(S, W, mag_eps=1e-9, floor=1e-5, log10=False):
    return _head(S, W, mag_eps, floor, log10, torch.float64)


def head32(S, W, mag_eps=1e-9, floor=1e-5, log10=False):
    return _head(S, W, mag_eps, floor, log10, torch.float32)


def _head_vjp(S, W, g, mel_branch, mag_eps, floor, log10, dt):
    S, W, g = torch.as_tensor(S).to(dt), torch.as_tensor(W).to(dt), torch.as_tensor(g).to(dt)
    live = torch.as_tensor(mel_branch).to(torch.float64) >= f32(floor)                # [B][T][M]
    re, im = S[..., 0], S[..., 1]
    mag = torch.sqrt(re * re + im * im + torch.tensor(f32(mag_eps), dtype=dt))
    mel = torch.matmul(W, mag).transpose(1, 2)                                        # this precision's own mel divides
    gm = torch.where(live, g / mel, torch.zeros((), dtype=dt))
    if log10:
        gm = gm / torch.tensor(np.log(10.0), dtype=dt)
    dmag = torch.matmul(W.t(), gm.transpose(1, 2))                                    # [B][n_bins][T]
    safe = torch.where(mag > 0, mag, torch.ones((), dtype=dt))
    return torch.where((mag > 0)[..., None], dmag[..., None] * S / safe[..., None], torch.zeros((), dtype=dt))


def head_vjp64(S, W, g, mel_branch, mag_eps=1e-9, floor=1e-5, log10=False):
    """G [B][n_bins][T][2] float64: gm = g / mel [/ ln 10] where mel_branch >= floor else 0; dmag = W^T gm; G = dmag (re, im) / mag, 0 where mag == 0"""
    return _head_vjp(S, W, g, mel_branch, mag_eps, floor, log10, torch.float64)


def head_vjp32(S, W, g, mel_branch, mag_eps=1e-9, floor=1e-5, log10=False):
    return _head_vjp(S, W, g, mel_branch, mag_eps, floor, log10, torch.float32)


def flavour(name, n_fft, hop, eps=1e-10):
    return SH._flavour(name, n_fft, hop, eps)


def stft_vjp(G, L, n_fft, hop, win, o, dtype=torch.float64):
    """G [B][n_bins][T][2] -> dL/dx [B][L] of the framing of flavour options `o` (before the clamp): the transpose on the PADDED signal by
    LH.vjp64 (float64) or LH.adjoint_matmul (float32), then the adjoint of the padding by autograd."""
    pl, pr = SH._pads(n_fft, o['center'], o['pad'])
    Lp = L + pl + pr
    if dtype == torch.float64:
        d = LH.vjp64(G, Lp, n_fft, hop, win, center=False)
    else:
        d = LH.adjoint_matmul(G, Lp, n_fft, hop, win, center=False, dtype=dtype)
    x = torch.zeros(d.shape[0], L, dtype=dtype, requires_grad=True)
    dx, = torch.autograd.grad(SH.padded(x * 1, n_fft, o['center'], o['pad_mode'], o['pad'], dtype), x, d.detach())
    return dx


def clamp_mask(x, o):
    x = torch.as_tensor(x)
    return ((x >= -1) & (x <= 1)).to(torch.float64) if o['clamp'] else torch.ones(x.shape, dtype=torch.float64)


def ref_loss64(x, target_or_y, basis, n_fft, hop, win, flavour_name='hifigan'):
    """mean |ref_logmel64(x) - target| as a float64 0-dim tensor (differentiable with respect to x): the target a waveform [B][L] or a log-mel
    [B][T][M]."""
    pred = SH.ref_logmel64(x, basis, flavour_name, n_fft, hop, win)[0]
    t = torch.as_tensor(target_or_y)
    tgt = SH.ref_logmel64(t, basis, flavour_name, n_fft, hop, win)[0] if t.dim() == 2 else t.double()
    return (pred - tgt.detach()).abs().mean()


def ref_loss32(x, y, basis, n_fft, hop, win):
    """The reference's operator sequence in float32 on the CPU (modules/hifigan/mel_utils.py:59-76 with return_complex=True, then l1_loss)."""
    import torch.nn.functional as F
    w = torch.hann_window(win)
    pad = (n_fft - hop) // 2
    basis = torch.as_tensor(basis).to(torch.float32)

    def mel(v):
        v = F.pad(torch.clamp(v.to(torch.float32), -1.0, 1.0)[:, None], (pad, pad), mode='reflect')[:, 0]
        S = torch.stft(v, n_fft, hop_length=hop, win_length=win, window=w, center=False, onesided=True, return_complex=True)
        mag = torch.sqrt(S.real ** 2 + S.imag ** 2 + 1e-9)
        return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5))
    return F.l1_loss(mel(x), mel(y).detach())


def signals(case, L, B):
    """The inputs of the GPU tests: (x, y) float32 [B][L]."""
    if case in ('near', 'loud'):
        y = SH.make_signal(L, seed=20, batch=B)
        x = y + 0.05 * torch.randn(y.shape, generator=torch.Generator().manual_seed(100))
        if case == 'loud':
            x, y = 2.5 * x, 2.5 * y
    elif case in ('far', 'silence', 'quiet'):
        x, y = SH.make_signal(L, seed=41, batch=B), SH.make_signal(L, seed=20, batch=B)
        if case == 'silence':
            x[:, L // 4:3 * L // 4] = 0
            y[-1, L // 3:2 * L // 3] = 0
        if case == 'quiet':
            x, y = 1e-4 * x, 1e-4 * y
    else:
        raise KeyError(case)
    return x.to(torch.float32), y.to(torch.float32)
