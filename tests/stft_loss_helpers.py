"""Test infrastructure of the STFT loss (include/dsv.h, section "STFT loss"): float64 restatements on the CPU built ONLY from torch.stft,
autograd and numpy - never from diffsinger_amd - with the float32 yardsticks and the error budgets the GPU bounds come from.

    ref_loss64 / ref_loss32      modules/parallel_wavegan/losses/stft_loss.py:12-153 from waveforms (float64 / the reference's float32 sequence)
    spectral64                   sc, mag, the analytic gradient G and its element-wise rounding budget from two given spectra
    vjp64                        the vector-Jacobian product of tests.stft_helpers.ref_stft64 by autograd
    adjoint_matmul               the same transpose as an explicit matrix product + overlap-add + padding fold, in a chosen dtype
                                 (float32: the yardstick of the family - the kernel may be 2 x its error; float64 with absolute=True: pushes
                                 an element-wise budget on G through |A|^T)"""
import numpy as np
import torch

from tests import stft_helpers as SH

CLAMP = 1e-7
U = 2.0 ** -24
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))          # configs/tts/pwg.yaml:77-82, the constructor defaults


def signals(case):
    """The inputs of the GPU tests: (x, y) float32 [B][L]."""
    if case == 'near':
        y = SH.make_signal(8000, seed=20, batch=2)
        x = y + 0.05 * torch.randn(y.shape, generator=torch.Generator().manual_seed(100))
    elif case == 'silence':
        x, y = SH.make_signal(8000, seed=41, batch=2), SH.make_signal(8000, seed=42, batch=2)
        x[:, 2000:5500] = 0
        y[1, 2500:5000] = 0
    elif case == 'short':
        x, y = SH.make_signal(1100, seed=41, batch=1), SH.make_signal(1100, seed=42, batch=1)
    elif case == 'odd':
        x, y = SH.make_signal(7999, seed=41, batch=3), SH.make_signal(7999, seed=42, batch=3)
    else:
        raise KeyError(case)
    return x.to(torch.float32), y.to(torch.float32)


def resolutions_of(case):
    return (RESOLUTIONS[1],) if case == 'short' else RESOLUTIONS


def magnitude(S):
    """stft_loss.py:26-31 on a complex spectrum [B][bins][T] (the transpose to [B][T][bins] changes neither norm nor mean)"""
    return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=CLAMP))


def loss_of_magnitudes(xm, ym):
    """stft_loss.py:52, :73"""
    sc = torch.linalg.norm((ym - xm).reshape(-1)) / torch.linalg.norm(ym.reshape(-1))
    mag = (torch.log(ym) - torch.log(xm)).abs().mean()
    return sc, mag


def ref_loss64(x, y, resolutions=RESOLUTIONS):
    """(sc, mag) float64 0-dim tensors, differentiable with respect to x: the mean over the resolutions of the loss of
    torch.stft(center=True, pad_mode='reflect', periodic Hann of win_length) in float64."""
    sc = mag = 0.0
    for n_fft, hop, win in resolutions:
        X = SH.ref_stft64(x, n_fft, hop, win, True, 'reflect')
        Y = SH.ref_stft64(y, n_fft, hop, win, True, 'reflect')
        s, m = loss_of_magnitudes(magnitude(X), magnitude(Y))
        sc, mag = sc + s, mag + m
    return sc / len(resolutions), mag / len(resolutions)


def ref_loss32(x, y, resolutions=RESOLUTIONS):
    """The reference's operator sequence in float32 on the CPU: torch.stft(x, fft, hop, win, hann_window(win)) with torch's defaults."""
    x, y = torch.as_tensor(x).to(torch.float32), torch.as_tensor(y).to(torch.float32)
    sc = mag = 0.0
    for n_fft, hop, win in resolutions:
        w = torch.hann_window(win)
        X = torch.stft(x, n_fft, hop, win, w, return_complex=True)
        Y = torch.stft(y, n_fft, hop, win, w, return_complex=True)
        s, m = loss_of_magnitudes(magnitude(X), magnitude(Y))
        sc, mag = sc + s, mag + m
    return sc / len(resolutions), mag / len(resolutions)


def grads_of(fn, x, y, resolutions):
    """((sc, mag), d sc / dx, d mag / dx) of a loss function of waveforms"""
    x = x.clone().requires_grad_(True)
    sc, mag = fn(x, y, resolutions)
    g_sc, = torch.autograd.grad(sc, x, retain_graph=True)
    g_mag, = torch.autograd.grad(mag, x)
    return (sc.detach(), mag.detach()), g_sc, g_mag


def spectral64(Xr, Yr, g_sc=1.0, g_mag=1.0):
    """From two spectra as real arrays [...][2] (any float dtype, evaluated in float64): a dict of
        sc, mag, G [...][2]        the loss and g_sc d sc / dX + g_mag d mag / dX (analytic: exactly 0 where X's clamp is active)
        kappa, mean_logs           the condition figures of the value bounds (issue text, test 2)
        tol [...]                  the element-wise budget of G per unit |(re, im)|: 16 u c + the full jump of a branch float32 can flip
        clamped                    the mask of elements whose gradient must be exactly 0 (those safely below the clamp)"""
    X, Y = np.asarray(Xr, dtype=np.float64), np.asarray(Yr, dtype=np.float64)
    Px, Py = X[..., 0] ** 2 + X[..., 1] ** 2, Y[..., 0] ** 2 + Y[..., 1] ** 2
    live = Px > CLAMP
    Pxc, Pyc = np.maximum(Px, CLAMP), np.maximum(Py, CLAMP)
    xm, ym = np.sqrt(Pxc), np.sqrt(Pyc)
    d = ym - xm
    n = Px.size
    S1, S2 = np.sqrt((d * d).sum()), np.sqrt((ym * ym).sum())
    lg = np.log(ym) - np.log(xm)
    sgn = np.sign(Pyc - Pxc)
    k_sc = -d / (xm * S1 * S2)                       # the live branch's coefficients, evaluated everywhere (Pxc > 0)
    k_mag = -sgn / (n * Pxc)
    coef = np.where(live, g_sc * k_sc + g_mag * k_mag, 0.0)
    c = np.where(live, abs(g_sc) * (np.abs(d) + xm + ym) / (xm * S1 * S2) + abs(g_mag) / (n * Pxc), 0.0)
    near_clamp = np.abs(Px - CLAMP) <= 4 * U * CLAMP
    diff = np.abs(Pxc - Pyc)
    near_sign = (diff > 0) & (diff <= 4 * U * np.maximum(Pxc, Pyc))
    jumps = near_clamp * np.abs(g_sc * k_sc + g_mag * k_mag) + near_sign * (2.0 * abs(g_mag) / (n * Pxc))
    return dict(sc=S1 / S2, mag=np.abs(lg).mean(), G=X * coef[..., None], tol=16 * U * c + jumps,
                kappa=(np.abs(d) * (xm + ym)).sum() / (d * d).sum(), mean_logs=(np.abs(np.log(xm)) + np.abs(np.log(ym))).mean(),
                clamped=~live & ~near_clamp, n_clamped=int((~live).sum()), n_flippable=int(near_clamp.sum() + near_sign.sum()))


def vjp64(G, L, n_fft, hop, win, center=True, pad_mode='constant'):
    """G [B][bins][T][2] -> float64 [B][L]: autograd through tests.stft_helpers.ref_stft64 (the imaginary cotangents of bin 0 and bin
    n_fft / 2 meet outputs that do not depend on the input)."""
    G = torch.as_tensor(G).to(torch.float64)
    x = torch.zeros(G.shape[0], L, dtype=torch.float64, requires_grad=True)
    S = torch.view_as_real(SH.ref_stft64(x, n_fft, hop, win, center, pad_mode))
    assert S.shape == G.shape, (S.shape, G.shape)
    dx, = torch.autograd.grad(S, x, G)
    return dx


def adjoint_matmul(G, L, n_fft, hop, win, center=True, pad_mode='constant', dtype=torch.float32, absolute=False):
    """The transpose as written out: frame_grad [B][T][n_fft] = G-as-rows @ basis^T (torch.matmul in `dtype`, the basis of
    stft_helpers.dft_basis32: float64 values rounded to float32), overlap-add in ascending frame order, the padding folded back by the
    adjoint of F.pad.  absolute=True uses |basis| (for budgets: G >= 0 then gives an upper bound of what element-wise errors of G can do)."""
    G = torch.as_tensor(G).to(dtype)
    B, bins, T, _ = G.shape
    D = SH.dft_basis32(n_fft, win).to(dtype)                                 # [n_fft][2][bins]
    if absolute:
        D = D.abs()
    D[:, 1, 0] = 0                                                           # Im of bin 0 and of bin n_fft / 2 do not depend on the signal
    D[:, 1, n_fft // 2] = 0
    rows = G.permute(0, 2, 3, 1).reshape(B, T, 2 * bins)                     # [B][T][(re | im) x bins]
    fg = torch.matmul(rows, D.reshape(n_fft, 2 * bins).t().contiguous())     # [B][T][n_fft]
    pl, pr = SH._pads(n_fft, center, None)
    buf = torch.zeros(B, L + pl + pr, dtype=dtype)
    for f in range(T):
        buf[:, f * hop:f * hop + n_fft] += fg[:, f]
    x = torch.zeros(B, L, dtype=dtype, requires_grad=True)
    dx, = torch.autograd.grad(SH.padded(x, n_fft, center, pad_mode, None, dtype), x, buf)
    return dx
