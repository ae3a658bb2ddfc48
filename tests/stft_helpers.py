"""Test infrastructure of the STFT family (include/dsv.h, section "STFT"): float64 restatements on the CPU built ONLY from torch.stft /
torch.istft / torch.matmul / numpy - never from diffsinger_amd.stft - and the float32 yardstick the GPU bounds come from.

    ref_stft64                 torch.stft in float64 (explicit padding, then center=False)
    ref_denoise64              vocoders/vocoder_utils.py:7-15 as tests/test_vocoder_host.py:235-243 restates it
    ref_logmel64               data_gen/tts/data_gen_utils.py:122-134 ('pwg') / modules/hifigan/mel_utils.py:59-76 ('hifigan')
    ref_process_utterance64    data_gen_utils.py:122-147 with a given mel basis
    yardstick32                the same contraction as a float32 torch.matmul on the CPU against a basis built in float64 and rounded to
                               float32 HERE: it shares only the definition with the code under test.  Both it and the kernel are fp32 sums
                               of the same products in a different order; the GPU bound is 2 x its error against the float64 reference."""
import numpy as np
import torch
import torch.nn.functional as F


def make_signal(n, seed=4, batch=None, noise=0.1):
    """tests/test_vocoder_host.py:234: noise plus a sinusoid, amplitude ~ 0.4."""
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if batch is None else (batch, n)
    return (torch.randn(shape, generator=g) * noise + 0.3 * torch.sin(torch.arange(n) * 0.05)).to(torch.float32)


def window64(n_fft, win):
    w = torch.zeros(n_fft, dtype=torch.float64)
    lp = (n_fft - win) // 2
    w[lp:lp + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
    return w


def _pads(n_fft, center, pad):
    if pad is None:
        pad = n_fft // 2 if center else 0
    return (pad, pad) if isinstance(pad, int) else tuple(pad)


def padded(wav, n_fft, center, pad_mode, pad, dtype):
    """[B][L] -> [B][L + pl + pr] in `dtype` (zeros or torch's reflect)."""
    x = torch.as_tensor(wav).to(dtype)
    if x.dim() == 1:
        x = x[None]
    pl, pr = _pads(n_fft, center, pad)
    if pl or pr:
        x = F.pad(x[:, None], (pl, pr), mode=pad_mode)[:, 0]
    return x


def ref_stft64(wav, n_fft, hop, win, center=True, pad_mode='constant', pad=None):
    """complex128 [B][n_bins][n_frames]."""
    x = padded(wav, n_fft, center, pad_mode, pad, torch.float64)
    return torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=window64(n_fft, win), center=False, onesided=True, return_complex=True)


def ref_istft64(S, n_fft, hop, win, length=None):
    return torch.istft(S, n_fft, hop_length=hop, win_length=n_fft, window=window64(n_fft, win), center=True, length=length)


def ref_denoise64(wav, v, n_fft, hop, win):
    """float64 [hop (n_frames - 1)] of a 1-D waveform."""
    x = torch.as_tensor(wav).double().reshape(-1)
    S = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=window64(n_fft, win), center=True, pad_mode='constant', onesided=True,
                   return_complex=True)
    S = torch.polar(torch.clamp(S.abs() - v, min=0), S.angle())
    return torch.istft(S, n_fft, hop_length=hop, win_length=n_fft, window=window64(n_fft, win), center=True)


FLAVOURS = {
    'pwg': dict(center=True, pad_mode='constant', pad=None, clamp=False, mag_eps=0.0, floor=None, log10=True),
    'hifigan': dict(center=False, pad_mode='reflect', pad='half', clamp=True, mag_eps=1e-9, floor=1e-5, log10=False),
}


def _flavour(flavour, n_fft, hop, eps):
    o = dict(FLAVOURS[flavour])
    if o['pad'] == 'half':
        o['pad'] = (n_fft - hop) // 2
    if o['floor'] is None:
        o['floor'] = eps
    return o


def ref_logmel64(wav, basis, flavour, n_fft, hop, win, eps=1e-10):
    """(log-mel [B][T][M], linear mel [B][T][M], magnitude [B][T][n_bins]) in float64."""
    o = _flavour(flavour, n_fft, hop, eps)
    x = torch.as_tensor(wav).double()
    if o['clamp']:
        x = x.clamp(-1.0, 1.0)
    S = ref_stft64(x, n_fft, hop, win, o['center'], o['pad_mode'], o['pad'])
    mag = torch.sqrt(S.real ** 2 + S.imag ** 2 + o['mag_eps'])
    mel = torch.matmul(torch.as_tensor(basis).double(), mag)
    clipped = torch.clamp(mel, min=o['floor'])
    out = torch.log10(clipped) if o['log10'] else torch.log(clipped)
    return out.transpose(1, 2), mel.transpose(1, 2), mag.transpose(1, 2)


def ref_process_utterance64(wav, basis, n_fft, hop, win, eps=1e-10, min_level_db=-100, return_linear=False):
    """data_gen_utils.py:122-147 with a given mel basis: (wav padded on the right by librosa_pad_lr and cut to T * hop, mel [T][M]
    [, (20 log10(max(1e-5, |S|)) - min_level_db) / -min_level_db [T][n_bins]])."""
    wav = np.asarray(wav, dtype=np.float32).reshape(-1)
    out, _, mag = ref_logmel64(wav, basis, 'pwg', n_fft, hop, win, eps)
    mel = out[0].numpy()
    T = mel.shape[0]
    r_pad = (len(wav) // hop + 1) * hop - len(wav)                       # utils/audio.py:38-47, pad_sides = 1
    w = np.pad(wav, (0, r_pad), mode='constant', constant_values=0.0)[:T * hop]
    if not return_linear:
        return w, mel
    spc = 20 * np.log10(np.maximum(1e-5, mag[0].numpy()))
    return w, mel, (spc - min_level_db) / -min_level_db


def dft_basis32(n_fft, win):
    """[n_fft][2][n_bins] float32: w[n] cos(2 pi k n / N), -w[n] sin(2 pi k n / N), evaluated in float64 with the angle reduced exactly."""
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % n_fft).astype(np.float64) / n_fft
    w = window64(n_fft, win).numpy()[:, None]
    return torch.from_numpy(np.stack([w * np.cos(ang), -w * np.sin(ang)], axis=1).astype(np.float32))


def yardstick32(wav, n_fft, hop, win, center=True, pad_mode='constant', pad=None, basis=None, flavour=None, eps=1e-10):
    """The forward contraction in float32 on the CPU (torch.matmul).  Without `basis`: complex64 [B][n_bins][T].  With a mel basis and a
    flavour: (log-mel, linear mel, magnitude) float32, [B][T][.]."""
    o = None
    x = torch.as_tensor(wav).to(torch.float32)
    if flavour is not None:
        o = _flavour(flavour, n_fft, hop, eps)
        center, pad_mode, pad = o['center'], o['pad_mode'], o['pad']
        if o['clamp']:
            x = x.clamp(-1.0, 1.0)
    x = padded(x, n_fft, center, pad_mode, pad, torch.float32)
    frames = x.unfold(1, n_fft, hop).contiguous()                        # [B][T][n_fft]
    D = dft_basis32(n_fft, win).reshape(n_fft, -1)                       # [n_fft][2 n_bins]
    Y = torch.matmul(frames, D).reshape(frames.shape[0], frames.shape[1], 2, -1)
    re, im = Y[:, :, 0], Y[:, :, 1]
    if flavour is None:
        return torch.complex(re, im).transpose(1, 2)
    mag = torch.sqrt(re * re + im * im + np.float32(o['mag_eps']))
    mel = torch.matmul(mag, torch.as_tensor(basis).to(torch.float32).t())
    clipped = torch.clamp(mel, min=float(np.float32(o['floor'])))
    out = torch.log10(clipped) if o['log10'] else torch.log(clipped)
    return out, mel, mag
