"""STFT on the device: framed real DFT, inverse with overlap-add, the spectral-subtraction post-filter and the log-mel analysis - the
operators of include/dsv.h, section "STFT" (kernels: csrc/voc_stft.hpp), on torch device tensors, and the `wav2spec` half of the
reference's vocoder interface built on them (vocoders/base_vocoder.py:22-39; vocoders/pwg.py:105-122 -> data_gen/tts/data_gen_utils.py:93-147).

    stft_op / istft_op       librosa.stft / librosa.istft, torch.stft / torch.istft
    denoise_op               vocoders/vocoder_utils.py:7-15 (the post-filter of HifiGAN.spec2wav), waveform in, waveform out, on the device
    logmel_op                data_gen_utils.py:122-134 ('pwg') and modules/hifigan/mel_utils.py:59-76 ('hifigan'); differentiable with respect
                             to the waveform (include/dsv.h, section "Mel loss"; kernels: csrc/voc_mel.hpp)
    spec_logmel_op           the head of that analysis on a given spectrum (magnitude, mel product, log), differentiable with respect to it
    mel_filterbank           librosa.filters.mel (Slaney scale and normalisation), restated: see its docstring
    wav2spec, wav2spec_batch PWG.wav2spec / HifiGAN.wav2spec (static methods of the vocoder classes)

torch is plumbing (buffers, streams).  There is no CPU path: the operators raise when the tensors are not on the MI355X.  Argument errors are
raised on the host (ValueError) before anything is enqueued; the C ABI refuses the same cases again (DSD_ERR_INVALID)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

SUPPORTED_N_FFT = (256, 512, 1024, 2048)
MAX_MEL_BINS = 128
_PAD_MODES = {'constant': 0, 'reflect': 1}
_BASES: dict = {}
_ADJ_BASES: dict = {}
_MEL_BASES: dict = {}


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _check_geometry(n_fft, hop, win):
    if n_fft not in SUPPORTED_N_FFT:
        raise ValueError(f'n_fft={n_fft} is not supported: one of {SUPPORTED_N_FFT}')
    if not isinstance(hop, (int, np.integer)) or not 1 <= hop <= n_fft:
        raise ValueError(f'hop={hop} must be an integer in [1, n_fft={n_fft}]')
    if not isinstance(win, (int, np.integer)) or not 1 <= win <= n_fft:
        raise ValueError(f'win_length={win} must be an integer in [1, n_fft={n_fft}]')


def _rows(wav: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
        raise RuntimeError(f'{what}: needs a device tensor (there is no CPU path)')
    if wav.dim() == 1:
        wav = wav[None]
    if wav.dim() != 2 or wav.shape[0] < 1 or wav.shape[0] > 65535 or wav.shape[1] < 1:
        raise ValueError(f'{what}: waveform must be [B][L] with 1 <= B <= 65535 and L >= 1, got {tuple(wav.shape)}')
    return wav.to(torch.float32).contiguous()


def _lengths(lengths, B, dev):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f'lengths must be [B={B}], got {tuple(lengths.shape)}')
    return lengths


def _pads(n_fft, center, pad):
    if pad is None:
        pad = n_fft // 2 if center else 0
    pl, pr = (pad, pad) if isinstance(pad, (int, np.integer)) else pad
    if pl < 0 or pr < 0:
        raise ValueError(f'padding ({pl}, {pr}) must not be negative')
    return int(pl), int(pr)


def n_frames(L: int, n_fft: int, hop: int, pad_l: int, pad_r: int) -> int:
    """1 + (L + pad_l + pad_r - n_fft) // hop; ValueError when the padded signal is shorter than one frame."""
    if L + pad_l + pad_r < n_fft:
        raise ValueError(f'signal shorter than one frame: L={L} + padding {pad_l} + {pad_r} < n_fft={n_fft}')
    return 1 + (L + pad_l + pad_r - n_fft) // hop


def bases(device, n_fft: int, win_length: int):
    """(forward, inverse) packed bases of (n_fft, win_length) on `device`, built once by the library (dsv_stft_make_basis, float64 on the
    device) and cached.  The one-time build is refused inside a graph capture: call the operator (or this) once before capturing - the
    warm-up calls of GraphedForward do."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), n_fft, win_length)
    hit = _BASES.get(key)
    if hit is not None:
        return hit
    _check_geometry(n_fft, 1, win_length)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f'the STFT basis of (n_fft={n_fft}, win_length={win_length}) is not built yet and cannot be built inside a graph '
                           f'capture: call diffsinger_amd.stft.bases(device, {n_fft}, {win_length}) first')
    lib = _lib.load()
    dev = torch.device('cuda', key[0])
    fwd = torch.empty(lib.dsv_stft_basis_floats(n_fft, 0), device=dev, dtype=torch.float32)
    inv = torch.empty(lib.dsv_stft_basis_floats(n_fft, 1), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.dsv_stft_make_basis(n_fft, win_length, fwd.data_ptr(), inv.data_ptr(), _stream(dev)), 'dsv_stft_make_basis')
    torch.cuda.current_stream(dev).synchronize()          # one-time: the buffers are used from any stream afterwards
    _BASES[key] = (fwd, inv)
    return fwd, inv


def adjoint_basis(device, n_fft: int, win_length: int):
    """The transposed forward basis of (n_fft, win_length) on `device` (dsv_stft_make_adjoint_basis), built once and cached like `bases`: the
    build is refused inside a graph capture - a differentiable stft_op call builds it in its FORWARD, so one warm-up call is enough."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), n_fft, win_length)
    hit = _ADJ_BASES.get(key)
    if hit is not None:
        return hit
    _check_geometry(n_fft, 1, win_length)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f'the adjoint STFT basis of (n_fft={n_fft}, win_length={win_length}) is not built yet and cannot be built inside a graph '
                           f'capture: call diffsinger_amd.stft.adjoint_basis(device, {n_fft}, {win_length}) first')
    lib = _lib.load()
    dev = torch.device('cuda', key[0])
    adj = torch.empty(lib.dsv_stft_basis_floats(n_fft, 2), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.dsv_stft_make_adjoint_basis(n_fft, win_length, adj.data_ptr(), _stream(dev)), 'dsv_stft_make_adjoint_basis')
    torch.cuda.current_stream(dev).synchronize()          # one-time: the buffer is used from any stream afterwards
    _ADJ_BASES[key] = adj
    return adj


def _stft_launch(x, lens, n_fft, hop, win_length, pl, pr, pad_mode, subtract, fc):
    """dsv_stft on validated arguments: x [B][L] float32 contiguous -> float32 [B][n_bins][n_frames][2]"""
    B, L = x.shape
    T = n_frames(L, n_fft, hop, pl, pr)
    fwd, _ = bases(x.device, n_fft, win_length)
    spec = torch.empty(B, n_fft // 2 + 1, T, 2, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.dsv_stft(x.data_ptr(), lens.data_ptr() if lens is not None else None, fwd.data_ptr(), spec.data_ptr(),
                                fc.data_ptr() if fc is not None else None, B, L, n_fft, hop, pl, pr, _PAD_MODES[pad_mode],
                                0 if subtract is None else 1, 0.0 if subtract is None else float(subtract), _stream(x.device)), 'dsv_stft')
    return spec


def stft_op(wav, *, n_fft, hop, win_length=None, center=True, pad_mode='constant', pad=None, lengths=None, subtract=None, return_frames=False):
    """wav [B][L] (or [L]) -> complex64 [B][n_fft / 2 + 1][n_frames], torch.stft's layout.  center: n_fft / 2 of padding per side (`pad`, an int
    or (left, right), overrides the amount); pad_mode 'constant' (zeros) or 'reflect'.  lengths [B]: valid samples per row - frames beyond a
    row's count are exactly 0.  subtract=v fuses S * max(|S| - v, 0) / |S| (the unfiltered spectrum is never written).  return_frames: also
    the rows' valid frame counts (int32 [B], device).
    A waveform that requires grad makes the call differentiable: its backward is the adjoint STFT (diffsinger_amd.stft_loss.stft_adjoint_op);
    subtract= and lengths= have no gradient (NotImplementedError)."""
    win_length = n_fft if win_length is None else win_length
    _check_geometry(n_fft, hop, win_length)
    if pad_mode not in _PAD_MODES:
        raise ValueError(f"pad_mode={pad_mode!r}: 'constant' or 'reflect'")
    x = _rows(wav, 'stft_op')
    B, L = x.shape
    pl, pr = _pads(n_fft, center, pad)
    if pad_mode == 'reflect' and max(pl, pr) >= L:
        raise ValueError(f'reflect padding ({pl}, {pr}) must be smaller than the signal (L={L})')
    n_frames(L, n_fft, hop, pl, pr)
    if subtract is not None and not (subtract >= 0 and np.isfinite(subtract)):
        raise ValueError(f'subtract={subtract} must be finite and >= 0')
    lens = _lengths(lengths, B, x.device)
    fc = torch.empty(B, device=x.device, dtype=torch.int32) if return_frames else None
    if x.requires_grad and torch.is_grad_enabled():
        if subtract is not None or lengths is not None:
            raise NotImplementedError('stft_op: subtract= and lengths= have no gradient (detach the waveform, or call it without them)')
        from .stft_loss import StftFunction
        spec = StftFunction.apply(x, n_fft, hop, win_length, pl, pr, pad_mode, fc)
    else:
        spec = _stft_launch(x, lens, n_fft, hop, win_length, pl, pr, pad_mode, subtract, fc)
    out = torch.view_as_complex(spec)
    return (out, fc) if return_frames else out


def istft_op(spec, *, n_fft, hop, win_length=None, center=True, length=None, frame_counts=None):
    """complex64 [B][n_fft / 2 + 1][n_frames] -> wav [B][length]: librosa.istft (inverse DFT x synthesis window, overlap-add in ascending frame
    order, division by the window sum-of-squares where it exceeds FLT_MIN, n_fft / 2 trimmed per side when center).  length defaults to
    n_fft + hop (n_frames - 1) [- 2 (n_fft / 2)]; samples beyond a row's signal (frame_counts [B]) are 0."""
    win_length = n_fft if win_length is None else win_length
    _check_geometry(n_fft, hop, win_length)
    if not isinstance(spec, torch.Tensor) or not spec.is_cuda:
        raise RuntimeError('istft_op: needs a device tensor (there is no CPU path)')
    if spec.dim() == 2:
        spec = spec[None]
    if spec.dim() != 3 or spec.shape[1] != n_fft // 2 + 1 or spec.shape[2] < 1 or not 1 <= spec.shape[0] <= 65535 or not spec.is_complex():
        raise ValueError(f'istft_op: spectrum must be complex [B][{n_fft // 2 + 1}][n_frames], got {tuple(spec.shape)} {spec.dtype}')
    s = torch.view_as_real(spec.to(torch.complex64).contiguous())
    B, _, T, _ = s.shape
    lib = _lib.load()
    if length is None:
        length = int(lib.dsv_istft_samples(T, n_fft, hop, 1 if center else 0))
    if length < 1:
        raise ValueError(f'istft_op: nothing left of {T} frame(s) after trimming n_fft / 2 per side')
    fcs = _lengths(frame_counts, B, s.device)
    _, inv = bases(s.device, n_fft, win_length)
    ws = torch.empty(lib.dsv_istft_workspace_floats(B, T, n_fft), device=s.device, dtype=torch.float32)
    out = torch.empty(B, length, device=s.device, dtype=torch.float32)
    with torch.cuda.device(s.device):
        _lib.check(lib.dsv_istft(s.data_ptr(), fcs.data_ptr() if fcs is not None else None, inv.data_ptr(), ws.data_ptr(), out.data_ptr(), B, T,
                                 length, n_fft, hop, 1 if center else 0, _stream(s.device)), 'dsv_istft')
    return out


def denoise_op(wav_dev, v, *, fft_size, hop_size, win_size, lengths=None):
    """vocoders/vocoder_utils.py:7-15 on the device: centred STFT (zero padding) with the spectral subtraction fused, inverse STFT.  wav
    [B][L] -> [B][hop (n_frames - 1)], n_frames = 1 + L // hop: the length diffsinger_amd.vocoder.denoise returns; with lengths [B] a row is
    filtered over its own valid samples and 0 behind them."""
    x = _rows(wav_dev, 'denoise_op')
    spec, fc = stft_op(x, n_fft=fft_size, hop=hop_size, win_length=win_size, center=True, pad_mode='constant', lengths=lengths,
                       subtract=float(v), return_frames=True)
    T = spec.shape[2]
    if T < 2:
        raise ValueError(f'denoise_op: a waveform of {x.shape[1]} sample(s) is shorter than one hop ({hop_size})')
    return istft_op(spec, n_fft=fft_size, hop=hop_size, win_length=win_size, center=True, length=hop_size * (T - 1),
                    frame_counts=fc if lengths is not None else None)


_FLAVOURS = {
    # data_gen/tts/data_gen_utils.py:122-134
    'pwg': dict(center=True, pad_mode='constant', clamp=False, mag_eps=0.0, log10=True),
    # modules/hifigan/mel_utils.py:59-76
    'hifigan': dict(center=False, pad_mode='reflect', clamp=True, mag_eps=1e-9, floor=1e-5, log10=False),
}


def logmel_op(wav_dev, mel_basis, *, n_fft, hop, win_length=None, flavour='pwg', eps=1e-10, lengths=None, return_linear=False,
              return_frames=False, **override):
    """Log-mel analysis in one launch: wav [B][L] -> [B][n_frames][M] (frames beyond a row's valid count exactly 0).  mel_basis: device float32
    [M][n_fft / 2 + 1], M <= 128 - data of the caller (librosa.filters.mel(...) or mel_filterbank).
    flavour 'pwg': centred, zero padding n_fft / 2, log10(max(mel, eps));  'hifigan': input clamped to [-1, 1], reflect padding
    (n_fft - hop) / 2, sqrt(. + 1e-9), ln(max(mel, 1e-5)).  Any of center, pad_mode, pad, clamp, mag_eps, floor, log10 may be overridden.
    return_linear: also the magnitude [B][n_frames][n_bins]; return_frames: also the rows' valid frame counts.
    A waveform that requires grad makes the call differentiable (one autograd node): dsv_mel_spectrum -> dsv_mel_head forward, and backward
    dsv_mel_head_backward -> dsv_stft_adjoint with the same padding -> dsv_mel_clamp_backward (flavours that clamp only); the gradient is exactly
    0 at floored cells and behind clamped samples.  lengths=, return_linear= and return_frames= have no gradient (NotImplementedError).  Without
    a gradient the call is the single fused launch."""
    if flavour not in _FLAVOURS:
        raise ValueError(f'flavour={flavour!r}: one of {sorted(_FLAVOURS)}')
    win_length = n_fft if win_length is None else win_length
    _check_geometry(n_fft, hop, win_length)
    o = dict(_FLAVOURS[flavour])
    o.setdefault('floor', eps)
    if flavour == 'hifigan':
        o['pad'] = (n_fft - hop) // 2
    unknown = set(override) - {'center', 'pad_mode', 'pad', 'clamp', 'mag_eps', 'floor', 'log10'}
    if unknown:
        raise TypeError(f'logmel_op: unknown argument(s) {sorted(unknown)}')
    o.update(override)
    if o['pad_mode'] not in _PAD_MODES:
        raise ValueError(f"pad_mode={o['pad_mode']!r}: 'constant' or 'reflect'")
    if not isinstance(mel_basis, torch.Tensor) or mel_basis.dim() != 2 or mel_basis.shape[1] != n_fft // 2 + 1:
        raise ValueError(f'mel_basis must be a tensor [M][{n_fft // 2 + 1}]')
    M = mel_basis.shape[0]
    if not 1 <= M <= MAX_MEL_BINS:
        raise ValueError(f'M={M} mel bins: at most {MAX_MEL_BINS} are supported')
    if not (o['floor'] > 0 and o['mag_eps'] >= 0):
        raise ValueError(f"floor={o['floor']} must be > 0 and mag_eps={o['mag_eps']} >= 0")
    grad = isinstance(wav_dev, torch.Tensor) and wav_dev.requires_grad and torch.is_grad_enabled()
    if grad:                                              # before a device is asked for: these hold on a host without one
        if lengths is not None or return_linear or return_frames:
            raise NotImplementedError('logmel_op: lengths=, return_linear= and return_frames= have no gradient (detach the waveform, or call it '
                                      'without them)')
        if mel_basis.requires_grad:
            raise NotImplementedError('logmel_op: no gradient with respect to the mel basis (detach it)')
    x = _rows(wav_dev, 'logmel_op')
    B, L = x.shape
    pl, pr = _pads(n_fft, o['center'], o.get('pad'))
    if o['pad_mode'] == 'reflect' and max(pl, pr) >= L:
        raise ValueError(f'reflect padding ({pl}, {pr}) must be smaller than the signal (L={L})')
    T = n_frames(L, n_fft, hop, pl, pr)
    if not mel_basis.is_cuda:
        raise RuntimeError('logmel_op: mel_basis must be a device tensor (there is no CPU path)')
    mb = mel_basis.detach().to(device=x.device, dtype=torch.float32).contiguous()
    if grad:
        return LogmelFunction.apply(x, mb, n_fft, hop, win_length, pl, pr, o['pad_mode'], bool(o['clamp']), float(o['mag_eps']), float(o['floor']),
                                    bool(o['log10']))
    lens = _lengths(lengths, B, x.device)
    fwd, _ = bases(x.device, n_fft, win_length)
    out = torch.empty(B, T, M, device=x.device, dtype=torch.float32)
    lin = torch.empty(B, T, n_fft // 2 + 1, device=x.device, dtype=torch.float32) if return_linear else None
    fc = torch.empty(B, device=x.device, dtype=torch.int32) if return_frames else None
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.dsv_logmel(x.data_ptr(), lens.data_ptr() if lens is not None else None, fwd.data_ptr(), mb.data_ptr(), out.data_ptr(),
                                  lin.data_ptr() if lin is not None else None, fc.data_ptr() if fc is not None else None, B, L, n_fft, hop, pl, pr,
                                  _PAD_MODES[o['pad_mode']], 1 if o['clamp'] else 0, M, float(o['mag_eps']), float(o['floor']),
                                  1 if o['log10'] else 0, _stream(x.device)), 'dsv_logmel')
    res = (out,) + ((lin,) if return_linear else ()) + ((fc,) if return_frames else ())
    return res[0] if len(res) == 1 else res


# ------------------------------------------------------------------------------------------------------------------------------------
# the differentiable chain (include/dsv.h, section "Mel loss"; kernels: csrc/voc_mel.hpp)
# ------------------------------------------------------------------------------------------------------------------------------------
def _spectrum_launch(x, n_fft, hop, win_length, pl, pr, pad_mode, clamp):
    """dsv_mel_spectrum on validated arguments: dsv_stft's launch reading clip(x, -1, 1) when `clamp` -> float32 [B][n_bins][n_frames][2]"""
    B, L = x.shape
    T = n_frames(L, n_fft, hop, pl, pr)
    fwd, _ = bases(x.device, n_fft, win_length)
    spec = torch.empty(B, n_fft // 2 + 1, T, 2, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dsv_mel_spectrum(x.data_ptr(), fwd.data_ptr(), spec.data_ptr(), B, L, n_fft, hop, pl, pr, _PAD_MODES[pad_mode],
                                                1 if clamp else 0, _stream(x.device)), 'dsv_mel_spectrum')
    return spec


def _head_launch(S, mb, mag_eps, floor, log10):
    """dsv_mel_head on validated arguments: S float32 [B][n_bins][T][2], mb float32 [M][n_bins], both contiguous -> (log-mel, linear mel) [B][T][M]"""
    B, n_bins, T, _ = S.shape
    M = mb.shape[0]
    out = torch.empty(B, T, M, device=S.device, dtype=torch.float32)
    mel = torch.empty(B, T, M, device=S.device, dtype=torch.float32)
    with torch.cuda.device(S.device):
        _lib.check(_lib.load().dsv_mel_head(S.data_ptr(), mb.data_ptr(), out.data_ptr(), mel.data_ptr(), B, T, 2 * (n_bins - 1), M, mag_eps, floor,
                                            1 if log10 else 0, _stream(S.device)), 'dsv_mel_head')
    return out, mel


def _head_backward_launch(S, mb, g, mel, mag_eps, floor, log10):
    """dsv_mel_head_backward: the cotangent g [B][T][M] of the log-mel -> G [B][n_bins][T][2]"""
    B, n_bins, T, _ = S.shape
    G = torch.empty_like(S)
    with torch.cuda.device(S.device):
        _lib.check(_lib.load().dsv_mel_head_backward(S.data_ptr(), mb.data_ptr(), g.data_ptr(), mel.data_ptr(), G.data_ptr(), B, T, 2 * (n_bins - 1),
                                                     mb.shape[0], mag_eps, floor, 1 if log10 else 0, _stream(S.device)), 'dsv_mel_head_backward')
    return G


class MelHeadFunction(torch.autograd.Function):
    """spec_logmel_op: one launch each way.  S float32 [B][n_bins][T][2] contiguous -> (log-mel, linear mel); the linear mel is saved for the
    backward and carries no gradient."""

    @staticmethod
    def forward(ctx, S, mb, mag_eps, floor, log10):
        out, mel = _head_launch(S, mb, mag_eps, floor, log10)
        ctx.save_for_backward(S, mb, mel)
        ctx.consts = (mag_eps, floor, log10)
        ctx.mark_non_differentiable(mel)
        return out, mel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_mel):
        S, mb, mel = ctx.saved_tensors
        return _head_backward_launch(S, mb, g.to(torch.float32).contiguous(), mel, *ctx.consts), None, None, None, None


class LogmelFunction(torch.autograd.Function):
    """logmel_op with a gradient: forward dsv_mel_spectrum -> dsv_mel_head; backward dsv_mel_head_backward -> dsv_stft_adjoint (the same padding)
    -> dsv_mel_clamp_backward (only when the flavour clamps).  x float32 [B][L] -> [B][n_frames][M]."""

    @staticmethod
    def forward(ctx, x, mb, n_fft, hop, win_length, pl, pr, pad_mode, clamp, mag_eps, floor, log10):
        adjoint_basis(x.device, n_fft, win_length)            # here, not in backward: a warm-up FORWARD is then enough before a capture
        S = _spectrum_launch(x, n_fft, hop, win_length, pl, pr, pad_mode, clamp)
        out, mel = _head_launch(S, mb, mag_eps, floor, log10)
        ctx.save_for_backward(x, S, mb, mel)
        ctx.consts = (mag_eps, floor, log10)
        ctx.geometry = (x.shape[1], n_fft, hop, win_length, pl, pr, pad_mode)
        ctx.clamp = clamp
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .stft_loss import _adjoint_launch
        x, S, mb, mel = ctx.saved_tensors
        G = _head_backward_launch(S, mb, g.to(torch.float32).contiguous(), mel, *ctx.consts)
        dx = _adjoint_launch(G, *ctx.geometry)
        if ctx.clamp:
            with torch.cuda.device(x.device):
                _lib.check(_lib.load().dsv_mel_clamp_backward(x.data_ptr(), dx.data_ptr(), dx.data_ptr(), dx.numel(), _stream(x.device)),
                           'dsv_mel_clamp_backward')
        return (dx,) + (None,) * 11


def spec_logmel_op(spec, mel_basis, *, mag_eps=1e-9, floor=1e-5, log10=False, return_linear_mel=False):
    """The head of the log-mel analysis on a given spectrum: spec complex64 [B][n_bins][T] (stft_op's result) or float [B][n_bins][T][2],
    mel_basis [M][n_bins] (M <= 128, data of the caller) -> log(max(mel_basis . sqrt(re^2 + im^2 + mag_eps), floor)) [B][T][M], natural or base
    10.  All bins are treated alike (an imaginary part stored at bin 0 or n_fft / 2 counts).  Differentiable with respect to `spec` only - one
    autograd node, one launch each way; the gradient is exactly 0 where the floor is active (it passes at equality) and where the magnitude is
    0.  A basis that requires grad raises NotImplementedError.  return_linear_mel: also the mel before the logarithm (no gradient)."""
    if not isinstance(spec, torch.Tensor) or not isinstance(mel_basis, torch.Tensor):
        raise ValueError('spec_logmel_op: spec and mel_basis must be tensors')
    if mel_basis.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('spec_logmel_op: no gradient with respect to the mel basis (detach it)')
    if mel_basis.dim() != 2 or (mel_basis.shape[1] - 1) * 2 not in SUPPORTED_N_FFT:
        raise ValueError(f'spec_logmel_op: mel_basis must be [M][n_fft / 2 + 1] with n_fft one of {SUPPORTED_N_FFT}, got {tuple(mel_basis.shape)}')
    M, n_bins = mel_basis.shape
    if not 1 <= M <= MAX_MEL_BINS:
        raise ValueError(f'M={M} mel bins: at most {MAX_MEL_BINS} are supported')
    if not (floor > 0 and mag_eps >= 0 and np.isfinite(floor) and np.isfinite(mag_eps)):
        raise ValueError(f'floor={floor} must be > 0 and mag_eps={mag_eps} >= 0, both finite')
    cplx = spec.is_complex()
    if cplx:
        if spec.dim() == 2:
            spec = spec[None]
        spec = torch.view_as_real(spec.to(torch.complex64).contiguous())
    if spec.dim() != 4 or spec.shape[3] != 2 or spec.shape[1] != n_bins or spec.shape[2] < 1 or not 1 <= spec.shape[0] <= 65535:
        raise ValueError(f'spec_logmel_op: spectrum must be complex [B][{n_bins}][T] or float [B][{n_bins}][T][2] with 1 <= B <= 65535, got '
                         f'{tuple(spec.shape)}')
    if not spec.is_cuda or not mel_basis.is_cuda:
        raise RuntimeError('spec_logmel_op: needs device tensors (there is no CPU path)')
    S = spec.to(torch.float32).contiguous()
    mb = mel_basis.detach().to(device=S.device, dtype=torch.float32).contiguous()
    if S.requires_grad and torch.is_grad_enabled():
        out, mel = MelHeadFunction.apply(S, mb, float(mag_eps), float(floor), bool(log10))
    else:
        out, mel = _head_launch(S, mb, float(mag_eps), float(floor), bool(log10))
    return (out, mel) if return_linear_mel else out


# ------------------------------------------------------------------------------------------------------------------------------------
# mel filterbank
# ------------------------------------------------------------------------------------------------------------------------------------
_F_SP = 200.0 / 3.0                 # Hz per mel below 1 kHz
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP  # = 15
_LOGSTEP = np.log(6.4) / 27.0       # per mel above 1 kHz


def hz_to_mel(f):
    """Slaney's auditory-toolbox scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (np.maximum(m, _MIN_LOG_MEL) - _MIN_LOG_MEL)), _F_SP * m)


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax) -> np.ndarray:
    """librosa 0.8's default filterbank, `librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)` (htk=False, norm='slaney'), written from its
    published definition: n_mels + 2 edges equally spaced on the Slaney mel scale between fmin and fmax; filter m is the triangle rising
    from edge m to edge m + 1 and falling to edge m + 2, sampled at the rfft bin frequencies k sr / n_fft; each triangle scaled by
    2 / (f[m + 2] - f[m]) (unit area).  Computed in float64, returned as float32 [n_mels][n_fft / 2 + 1].
    PARITY UNPINNED against librosa itself (absent here; librosa accumulates the weights in float32).  The operators take the basis as
    DATA: a caller who has librosa passes `librosa.filters.mel(...)` and gets the reference's numbers - the kernels' parity does not rest
    on this function."""
    if fmax is None:
        fmax = sr / 2.0
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    edges = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w.astype(np.float32)


def mel_basis_on(device, sr, n_fft, n_mels, fmin, fmax) -> torch.Tensor:
    """mel_filterbank(...) as a cached device tensor."""
    device = torch.device(device)
    key = (device.type, device.index, sr, n_fft, n_mels, fmin, fmax)
    if key not in _MEL_BASES:
        _MEL_BASES[key] = torch.from_numpy(mel_filterbank(sr, n_fft, n_mels, fmin, fmax)).to(device)
    return _MEL_BASES[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# wav2spec (vocoders/pwg.py:105-122 -> data_gen/tts/data_gen_utils.py:93-147)
# ------------------------------------------------------------------------------------------------------------------------------------
_WAV2SPEC_KEYS = ('fft_size', 'hop_size', 'win_size', 'audio_num_mel_bins', 'fmin', 'fmax', 'audio_sample_rate', 'min_level_db')


def _wav2spec_params(hp) -> dict:
    missing = [k for k in _WAV2SPEC_KEYS if k not in hp or hp[k] is None]
    if missing:
        raise KeyError(f'wav2spec: hparams lack {missing} (needed: {list(_WAV2SPEC_KEYS)}; wav2spec_eps defaults to 1e-10)')
    for k, pkg in (('loud_norm', 'pyloudnorm'), ('trim_long_sil', 'webrtcvad')):
        if hp.get(k):
            raise NotImplementedError(f"wav2spec: hparams['{k}'] needs {pkg} (not in this image, not rebuilt here): prepare the waveform first")
    sr = hp['audio_sample_rate']
    fmin, fmax = hp['fmin'], hp['fmax']
    return dict(n_fft=int(hp['fft_size']), hop=int(hp['hop_size']), win=int(hp['win_size']), M=int(hp['audio_num_mel_bins']), sr=sr,
                fmin=0 if fmin == -1 else fmin, fmax=sr / 2 if fmax == -1 else fmax, eps=float(hp.get('wav2spec_eps', 1e-10)),
                min_level_db=hp['min_level_db'])


def read_wav(path: str, sample_rate: int) -> np.ndarray:
    """A WAV file as mono float32 in [-1, 1).  The file must be AT `sample_rate`: the reference resamples with librosa's kaiser_best
    (librosa.core.load), which is not rebuilt here."""
    try:
        from scipy.io import wavfile
        sr, data = wavfile.read(path)
    except ImportError:
        import wave
        with wave.open(path, 'rb') as f:
            sr, width, ch = f.getframerate(), f.getsampwidth(), f.getnchannels()
            if width != 2:
                raise NotImplementedError(f'{path}: {8 * width}-bit PCM needs scipy (the stdlib reader handles 16-bit)')
            data = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2').reshape(-1, ch)
    if int(sr) != int(sample_rate):
        raise ValueError(f'{path} is sampled at {sr} Hz but audio_sample_rate is {sample_rate} Hz: resample it first (the reference resamples '
                         f'with librosa, which is not rebuilt here)')
    data = np.asarray(data)
    if data.dtype.kind == 'i':
        data = data.astype(np.float32) / float(1 << (8 * data.dtype.itemsize - 1))
    elif data.dtype.kind == 'u':
        data = (data.astype(np.float32) - 128.0) / 128.0
    data = data.astype(np.float32)
    return data.mean(axis=1).astype(np.float32) if data.ndim == 2 else data


def wav2spec_batch(wavs_dev, lengths=None):
    """The device-resident form of wav2spec: wavs [B][L] (device, at hparams['audio_sample_rate']) -> log10-mel [B][1 + L // hop][M] by the
    process-wide hparams, no host copy; rows shorter than L through lengths [B] (their frames beyond 1 + len // hop are 0)."""
    from .hparams import hparams
    q = _wav2spec_params(hparams)
    x = _rows(wavs_dev, 'wav2spec_batch')
    mb = mel_basis_on(x.device, q['sr'], q['n_fft'], q['M'], q['fmin'], q['fmax'])
    return logmel_op(x, mb, n_fft=q['n_fft'], hop=q['hop'], win_length=q['win'], flavour='pwg', eps=q['eps'], lengths=lengths)


def wav2spec(wav_fn, return_linear=False):
    """vocoders/pwg.py:105-122: (wav, mel [T, M]) or, return_linear, (wav, mel, spc [T, n_fft / 2 + 1]) - numpy float32 like the reference.
    wav = the input padded on the right (utils/audio.py librosa_pad_lr) and cut to T * hop, T = 1 + len // hop; mel = log10(max(eps,
    mel_basis @ |STFT|)); spc = (20 log10(max(1e-5, |STFT|)) - min_level_db) / -min_level_db (utils/audio.py:51-56).
    `wav_fn`: a float array, or the path of a mono-or-averaged WAV file at hparams['audio_sample_rate'] (another rate: ValueError).
    hparams['loud_norm'] / ['trim_long_sil']: NotImplementedError (pyloudnorm / webrtcvad are not here).  The analysis runs on the device."""
    from .hparams import hparams
    q = _wav2spec_params(hparams)
    if isinstance(wav_fn, str):
        wav = read_wav(wav_fn, q['sr'])
    else:
        wav = np.asarray(wav_fn, dtype=np.float32).reshape(-1)
    if not torch.cuda.is_available():
        raise RuntimeError('wav2spec: needs the MI355X (there is no CPU path)')
    x = torch.from_numpy(np.ascontiguousarray(wav)).cuda()[None]
    mb = mel_basis_on(x.device, q['sr'], q['n_fft'], q['M'], q['fmin'], q['fmax'])
    res = logmel_op(x, mb, n_fft=q['n_fft'], hop=q['hop'], win_length=q['win'], flavour='pwg', eps=q['eps'], return_linear=return_linear)
    mel = (res[0] if return_linear else res)[0].cpu().numpy()
    T = mel.shape[0]
    out = np.zeros(T * q['hop'], dtype=np.float32)
    out[:len(wav)] = wav
    if not return_linear:
        return out, mel
    spc = res[1][0].cpu().numpy()
    spc = 20 * np.log10(np.maximum(np.float32(1e-5), spc))
    spc = ((spc - q['min_level_db']) / -q['min_level_db']).astype(np.float32)
    return out, mel, spc
