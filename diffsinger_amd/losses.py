"""The training objective of FastSpeech2 on HIP: the mel terms (masked L1 + SSIM) and the duration terms (pdur / wdur / sdur) of
FastSpeech2Task.run_model (tasks/tts/fs2.py:111-283) and of the MIDI tasks (usr/diffsinger_task.py:279-389, :404-473), as autograd Functions on
the kernels of csrc/fs2_loss.hpp (include/dsf.h, "FastSpeech2 training objective").

    ssim(img1, img2, window_size=11, size_average=True)     drop-in for modules.commons.ssim.ssim on [B,1,H,W], W <= 128
    fs2_losses(output, sample, hp, variant='fs2' | 'midi', sil_ph_ids=None)   the reference's loss dict

Nothing here synchronises with the host: the word buffer is sized by the phone count, not by the data (the reference's `word_id.max()`), so a
whole training step can be captured as a graph.  The cwt terms (C / uv / f0_mean / f0_std) are one fused operator on the kernels of
csrc/fs2_cwt.hpp ("CWT pitch"); the frame- and phone-level pitch terms and the energy term act on [B, T] vectors and are torch expressions
on the device.  There is no CPU path: CPU tensors are refused."""
from __future__ import annotations


import torch
import torch.nn.functional as F

from . import _lib

MAX_BINS = 128          # bins of one mel frame the SSIM kernels hold in LDS
MAX_PHONES = 2048       # phones per utterance of the duration kernels


def _f32_rows(name, t):
    """[B, T, M] fp32 on the GPU with contiguous bins (the kernels read 4-byte elements: no alignment beyond the element's is needed)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f'{name}: a CUDA tensor is required (there is no CPU path)')
    if t.dtype != torch.float32:
        raise ValueError(f'{name}: float32 required, got {t.dtype}')
    if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] < 1 or not 1 <= t.shape[2] <= MAX_BINS:
        raise ValueError(f'{name}: [B, T, M] with 1 <= M <= {MAX_BINS} required, got {tuple(t.shape)}')
    if t.stride(2) != 1 and t.shape[2] > 1:
        t = t.contiguous()
    return t


class _MelLoss(torch.autograd.Function):
    """out = [lam_l1 L1, lam_ssim (1 - SSIM), mean S, count] (+ the SSIM map when asked for); dsf_mel_loss / dsf_mel_loss_bwd."""

    @staticmethod
    def forward(ctx, x, y, bias, weighted, terms, lam_l1, lam_ssim, want_map):
        lib = _lib.load()
        B, T, M = x.shape
        ws = torch.empty(int(lib.dsf_fs2_loss_workspace_floats(B, T, 0)), device=x.device, dtype=torch.float32)
        out = torch.empty(4, device=x.device, dtype=torch.float32)
        smap = torch.empty((B, T, M) if want_map else (0,), device=x.device, dtype=torch.float32)
        _lib.call('dsf_mel_loss', x.device, x.data_ptr(), x.stride(0), x.stride(1), y.data_ptr(), y.stride(0), y.stride(1), B, T, M, float(bias),
                  int(weighted), int(terms), float(lam_l1), float(lam_ssim), smap.data_ptr() if want_map else None, ws.data_ptr(), out.data_ptr())
        ctx.save_for_backward(x, y, out)
        ctx.cfg = (float(bias), int(weighted), int(terms), float(lam_l1), float(lam_ssim), bool(want_map))
        return out, smap

    @staticmethod
    def backward(ctx, g_out, g_map):
        x, y, out = ctx.saved_tensors
        bias, weighted, terms, lam_l1, lam_ssim, want_map = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        B, T, M = x.shape
        g = g_out[:3].contiguous()
        gm = g_map.contiguous() if (want_map and g_map is not None and g_map.numel()) else None
        dx = torch.empty((B, T, M), device=x.device, dtype=torch.float32)
        _lib.call('dsf_mel_loss_bwd', x.device, x.data_ptr(), x.stride(0), x.stride(1), y.data_ptr(), y.stride(0), y.stride(1), B, T, M, bias, weighted,
                  terms, lam_l1, lam_ssim, out.data_ptr(), g.data_ptr(), _lib.ptr(gm), dx.data_ptr())
        return dx, None, None, None, None, None, None, None


def mel_loss_terms(mel_out, target, *, bias=6.0, l1=True, ssim=True, lam_l1=1.0, lam_ssim=1.0):
    """[lam_l1 * l1_loss, lam_ssim * ssim_loss, mean S, count] of FastSpeech2Task (tasks/tts/fs2.py:160-178) in one kernel pass; a [4] tensor."""
    x, y = _f32_rows('mel_out', mel_out), _f32_rows('target', target)
    if x.shape != y.shape or x.device != y.device:
        raise ValueError(f'mel_out {tuple(x.shape)} and target {tuple(y.shape)} must have one shape and device')
    if y.requires_grad:
        raise NotImplementedError('the target gets no gradient')
    terms = (1 if l1 else 0) | (2 if ssim else 0)
    if not terms:
        raise ValueError('no term asked for')
    out, _ = _MelLoss.apply(x, y, bias, 1, terms, lam_l1, lam_ssim, False)
    return out


def ssim(img1, img2, window_size=11, size_average=True):
    """modules/commons/ssim.py:383-391 on the HIP kernels: img1 / img2 [B, 1, H, W] fp32 CUDA, W <= 128; the mean of the SSIM map
    (size_average) or the map [B, H, W] (= ssim_map.mean(1) of the single channel).  Gradient with respect to img1 only."""
    if window_size != 11:
        raise ValueError(f'ssim: window_size must be 11 (the Gaussian window of the kernels), got {window_size}')
    for n, t in (('img1', img1), ('img2', img2)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f'ssim: {n} must be [B, 1, H, W] (one channel), got {tuple(t.shape) if torch.is_tensor(t) else type(t)}')
    if img1.shape != img2.shape:
        raise ValueError(f'ssim: img1 {tuple(img1.shape)} and img2 {tuple(img2.shape)} differ in shape')
    if img2.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('ssim: no gradient with respect to img2 (the target)')
    x, y = _f32_rows('img1', img1[:, 0]), _f32_rows('img2', img2[:, 0])
    out, smap = _MelLoss.apply(x, y, 0.0, 0, 2, 0.0, 0.0, not size_average)
    return out[2] if size_average else smap


class _DurLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dur_pred, mel2ph, tokens, sil_ids, wdb, lam_ph, lam_word, lam_sent):
        lib = _lib.load()
        B, Tt = tokens.shape
        T = mel2ph.shape[1]
        ws = torch.empty(int(lib.dsf_fs2_loss_workspace_floats(B, Tt, 1)), device=dur_pred.device, dtype=torch.float32)
        out = torch.empty(3, device=dur_pred.device, dtype=torch.float32)
        args = (dur_pred.data_ptr(), mel2ph.data_ptr(), tokens.data_ptr(), _lib.ptr(sil_ids), int(sil_ids.numel()) if sil_ids is not None else 0,
                _lib.ptr(wdb), B, Tt, T, float(lam_ph), float(lam_word), float(lam_sent))
        _lib.call('dsf_dur_loss', dur_pred.device, *args, ws.data_ptr(), out.data_ptr())
        ctx.args = args
        ctx.save_for_backward(dur_pred, mel2ph, tokens, sil_ids if sil_ids is not None else ws[:0], wdb if wdb is not None else ws[:0], ws)
        return out

    @staticmethod
    def backward(ctx, g):
        dur_pred, _m, _t, _s, _w, ws = ctx.saved_tensors         # kept alive: the pointers in ctx.args are theirs
        grad = torch.empty_like(dur_pred)
        g = g.contiguous()
        _lib.call('dsf_dur_loss_bwd', dur_pred.device, *ctx.args, ws.data_ptr(), g.data_ptr(), grad.data_ptr())
        return grad, None, None, None, None, None, None, None


def _i64(name, t, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f'{name}: a CUDA tensor is required (there is no CPU path)')
    if t.dtype != torch.int64:
        t = t.long()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: shape {tuple(shape)} expected, got {tuple(t.shape)}')
    return t.contiguous()


def dur_loss_terms(dur_pred, mel2ph, txt_tokens, *, sil_ids=None, word_boundary=None, lam_ph=1.0, lam_word=1.0, lam_sent=1.0):
    """[pdur, wdur, sdur] of add_dur_loss with dur_loss 'mse' (tasks/tts/fs2.py:180-219 with sil_ids; usr/diffsinger_task.py:359-389 with
    word_boundary), each times its lambda; a [3] tensor."""
    if (sil_ids is None) == (word_boundary is None):
        raise ValueError('dur_loss_terms: exactly one of sil_ids (FastSpeech2Task) and word_boundary (the MIDI tasks)')
    if not torch.is_tensor(dur_pred) or not dur_pred.is_cuda or dur_pred.dtype != torch.float32 or dur_pred.dim() != 2:
        raise ValueError('dur_pred: a [B, T_txt] float32 CUDA tensor is required (there is no CPU path)')
    B, Tt = dur_pred.shape
    if not 1 <= Tt <= MAX_PHONES:
        raise ValueError(f'dur_pred: 1 <= T_txt <= {MAX_PHONES} required, got {Tt}')
    tok = _i64('txt_tokens', txt_tokens, (B, Tt))
    m2p = _i64('mel2ph', mel2ph)
    if m2p.dim() != 2 or m2p.shape[0] != B or m2p.shape[1] < 1:
        raise ValueError(f'mel2ph: [B, T] with B = {B} required, got {tuple(m2p.shape)}')
    sil = _i64('sil_ids', sil_ids) if sil_ids is not None else None
    wdb = _i64('word_boundary', word_boundary, (B, Tt)) if word_boundary is not None else None
    return _DurLoss.apply(dur_pred.contiguous(), m2p, tok, sil, wdb, lam_ph, lam_word, lam_sent)


class _CwtPitchLoss(torch.autograd.Function):
    """out = [C, uv, f0_mean, f0_std, sum nonpadding]; dsf_cwt_pitch_loss / dsf_cwt_pitch_loss_bwd."""

    @staticmethod
    def forward(ctx, pred, mean_pred, std_pred, spec, uv, mel2ph, mean_tgt, std_tgt, use_uv, l2, lam_f0, lam_uv):
        lib = _lib.load()
        B, T, Cp = pred.shape
        ws = torch.empty(int(lib.dsf_cwt_pitch_loss_workspace_floats()), device=pred.device, dtype=torch.float32)
        out = torch.empty(5, device=pred.device, dtype=torch.float32)
        args = (pred.data_ptr(), pred.stride(0), pred.stride(1), pred.stride(2), spec.data_ptr(), _lib.ptr(uv if use_uv else None),
                _lib.ptr(mel2ph if use_uv else None), mean_pred.data_ptr(), mean_tgt.data_ptr(), std_pred.data_ptr(), std_tgt.data_ptr(), B, T, Cp,
                int(use_uv), int(l2), float(lam_f0), float(lam_uv))
        _lib.call('dsf_cwt_pitch_loss', pred.device, *args, ws.data_ptr(), out.data_ptr())
        ctx.args = args
        ctx.save_for_backward(pred, mean_pred, std_pred, spec, uv if use_uv else spec, mel2ph if use_uv else spec, mean_tgt, std_tgt, out)
        return out

    @staticmethod
    def backward(ctx, g):
        pred, *_kept, out = ctx.saved_tensors                   # kept alive: the pointers in ctx.args are theirs
        B, T, Cp = pred.shape
        g4 = g[:4].contiguous()
        dp = torch.empty((B, T, Cp), device=pred.device, dtype=torch.float32)
        dmean = torch.empty(B, device=pred.device, dtype=torch.float32)
        dstd = torch.empty(B, device=pred.device, dtype=torch.float32)
        _lib.call('dsf_cwt_pitch_loss_bwd', pred.device, *ctx.args, out.data_ptr(), g4.data_ptr(), dp.data_ptr(), dmean.data_ptr(), dstd.data_ptr())
        return (dp, dmean, dstd) + (None,) * 9


def _f32_on(name, t, shape, dev):
    if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
        raise ValueError(f'{name}: a CUDA tensor on {dev} is required (there is no CPU path)')
    if t.dtype != torch.float32:
        raise ValueError(f'{name}: float32 required, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: shape {tuple(shape)} expected, got {tuple(t.shape)}')
    return t


def cwt_pitch_loss_terms(cwt_out, cwt_spec, uv, mel2ph, f0_mean_pred, f0_mean, f0_std_pred, f0_std, *, cwt_loss='l1', use_uv=True, lambda_f0=1.0,
                         lambda_uv=1.0):
    """[C, uv, f0_mean, f0_std] of the cwt branch of FastSpeech2Task.add_pitch_loss (tasks/tts/fs2.py:233-247), each times its lambda, from one
    pass over cwt_out: a [4] tensor (uv reads 0 without use_uv).  cwt_out: the cwt predictor's output [B, T, 10 (+ 1 with use_uv: the uv
    logit is the LAST channel)] fp32 with any strides; cwt_spec [B, T, 10]; uv [B, T] float; mel2ph [B, T] (nonpadding = mel2ph != 0); the four
    statistics [B].  Gradients: cwt_out (the whole tensor in one launch), f0_mean_pred, f0_std_pred."""
    if cwt_loss not in ('l1', 'l2'):
        raise NotImplementedError(f"cwt_pitch_loss_terms: cwt_loss {cwt_loss!r} (ssim goes through mel_loss_terms)")
    if not torch.is_tensor(cwt_out) or not cwt_out.is_cuda:
        raise ValueError('cwt_out: a CUDA tensor is required (there is no CPU path)')
    need = 11 if use_uv else 10
    if cwt_out.dtype != torch.float32 or cwt_out.dim() != 3 or cwt_out.shape[0] < 1 or cwt_out.shape[1] < 1 or cwt_out.shape[2] < need:
        raise ValueError(f'cwt_out: float32 [B, T, {need}+] required, got {cwt_out.dtype} {tuple(cwt_out.shape)}')
    B, T = cwt_out.shape[:2]
    dev = cwt_out.device
    spec = _f32_on('cwt_spec', cwt_spec, (B, T, 10), dev).contiguous()
    stats = [_f32_on(n, t, (B,), dev) for n, t in (('f0_mean_pred', f0_mean_pred), ('f0_std_pred', f0_std_pred), ('f0_mean', f0_mean), ('f0_std', f0_std))]
    if any(t.requires_grad for t in (spec, stats[2], stats[3])):
        raise NotImplementedError('cwt_pitch_loss_terms: the targets get no gradient')
    uv_c = m2p = None
    if use_uv:
        uv_c = _f32_on('uv', uv, (B, T), dev).contiguous()
        m2p = _i64('mel2ph', mel2ph, (B, T))
    out = _CwtPitchLoss.apply(cwt_out, stats[0].contiguous(), stats[1].contiguous(), spec, uv_c, m2p, stats[2].contiguous(), stats[3].contiguous(),
                              bool(use_uv), cwt_loss == 'l2', float(lambda_f0), float(lambda_uv))
    return out[:4]


def _cwt_loss_fusable(output, sample, hp) -> bool:
    """Plain CUDA fp32 tensors of the shapes the operator takes; anything else keeps the torch expressions (and their error messages)."""
    c = output['cwt']
    if not (torch.is_tensor(c) and c.is_cuda and c.dtype == torch.float32 and c.dim() == 3 and c.shape[2] == (11 if hp['use_uv'] else 10)
            and c.shape[0] >= 1 and c.shape[1] >= 1):
        return False
    B, T = c.shape[:2]
    want = [(sample['cwt_spec'], (B, T, 10)), (output['f0_mean'], (B,)), (output['f0_std'], (B,)), (sample['f0_mean'], (B,)), (sample['f0_std'], (B,))]
    if hp['use_uv']:
        want.append((sample['uv'], (B, T)))
        m = sample['mel2ph']
        if not (torch.is_tensor(m) and m.device == c.device and m.dtype == torch.int64 and tuple(m.shape) == (B, T)):
            return False
    return all(torch.is_tensor(t) and t.device == c.device and t.dtype == torch.float32 and tuple(t.shape) == s for t, s in want) and not any(
        t.requires_grad for t in (sample['cwt_spec'], sample['f0_mean'], sample['f0_std']))


def parse_mel_loss(spec: str) -> dict:
    """hparams['mel_loss'] -> {name: lambda} as FastSpeech2Task.__init__ builds it (tasks/tts/fs2.py:34-44)."""
    out = {}
    for item in spec.split('|'):
        if item == '':
            continue
        if ':' in item:
            name, lbd = item.split(':')
            out[name] = float(lbd)
        else:
            out[item] = 1.0
    return out


def sil_phone_ids(vocab) -> list:
    """The ids of TokenTextEncoder.sil_phonemes() (utils/text_encoder.py:303-304): tokens whose first character is not a letter."""
    return [i for i, p in enumerate(vocab) if not p[0].isalpha()]


def _masked_mean(v, mask):
    return (v * mask).sum() / mask.sum()


def fs2_losses(output: dict, sample: dict, hp: dict, *, variant: str = 'fs2', sil_ph_ids=None) -> dict:
    """The loss dict of the reference's run_model, same keys, same order, same lambdas:
        variant 'fs2'   FastSpeech2Task.run_model (tasks/tts/fs2.py:111-283): mel terms, then pdur (times lambda_ph_dur) / wdur / sdur with the
                        words of the silence phones `sil_ph_ids` (a list of token ids, or a CUDA int64 tensor)
        variant 'midi'  AuxDecoderMIDITask (usr/diffsinger_task.py:404-473; output has 'mel_out') or DiffSingerMIDITask (:279-389; output has
                        'diff_loss', stored as 'mel'): pdur (unscaled) / wdur / sdur with the words of sample['word_boundary']
    then f0 / uv / C / f0_mean / f0_std (use_pitch_embed) and e (use_energy_embed)."""
    if variant not in ('fs2', 'midi'):
        raise ValueError(f"variant must be 'fs2' or 'midi', got {variant!r}")
    if hp.get('dur_loss', 'mse') != 'mse':
        raise NotImplementedError(f"dur_loss {hp.get('dur_loss')!r}: only 'mse' (the reference runs no other: mog returns, crf needs the model's CRF)")
    if hp.get('use_pitch_embed') and hp.get('pitch_type') != 'ph' and hp.get('pitch_loss', 'l1') not in ('l1', 'l2'):
        raise NotImplementedError(f"pitch_loss {hp.get('pitch_loss')!r}: the reference computes no f0 loss for it (tasks/tts/fs2.py:260-261)")
    target = sample['mels']
    txt_tokens, mel2ph = sample['txt_tokens'], sample['mel2ph']
    losses = {}
    if variant == 'midi' and 'diff_loss' in output:
        losses['mel'] = output['diff_loss']
    else:
        lam = parse_mel_loss(hp['mel_loss'])
        bad = [k for k in lam if k not in ('l1', 'ssim')]
        if bad:
            raise NotImplementedError(f'mel_loss {bad}: the reference raises NotImplementedError for mse / gdl (tasks/tts/fs2.py:151-158)')
        t = mel_loss_terms(output['mel_out'], target, l1='l1' in lam, ssim='ssim' in lam, lam_l1=lam.get('l1', 0.0), lam_ssim=lam.get('ssim', 0.0))
        for k in lam:
            losses[k] = t[0] if k == 'l1' else t[1]
    # durations
    if variant == 'fs2':
        if sil_ph_ids is None:
            raise ValueError("variant 'fs2' needs sil_ph_ids (the ids of the phone encoder's sil_phonemes(), see sil_phone_ids)")
        sil = sil_ph_ids if torch.is_tensor(sil_ph_ids) else torch.tensor(list(sil_ph_ids), dtype=torch.int64)
        sil = sil.to(txt_tokens.device)
        d = dur_loss_terms(output['dur'], mel2ph, txt_tokens, sil_ids=sil, lam_ph=hp['lambda_ph_dur'], lam_word=hp['lambda_word_dur'],
                           lam_sent=hp['lambda_sent_dur'])
    else:
        d = dur_loss_terms(output['dur'], mel2ph, txt_tokens, word_boundary=sample['word_boundary'], lam_ph=1.0, lam_word=hp['lambda_word_dur'],
                           lam_sent=hp['lambda_sent_dur'])
    losses['pdur'] = d[0]
    if hp['lambda_word_dur'] > 0:
        losses['wdur'] = d[1]
    if hp['lambda_sent_dur'] > 0:
        losses['sdur'] = d[2]
    if hp.get('use_pitch_embed'):
        _add_pitch_loss(output, sample, hp, losses)
    if hp.get('use_energy_embed'):
        energy = sample['energy']
        losses['e'] = _masked_mean(F.mse_loss(output['energy_pred'], energy, reduction='none'), (energy != 0).float()) * hp['lambda_energy']
    return losses


def _add_pitch_loss(output, sample, hp, losses):
    """FastSpeech2Task.add_pitch_loss / add_f0_loss / cwt_loss (tasks/tts/fs2.py:221-277) as device tensor expressions."""
    if hp['pitch_type'] == 'ph':
        nonpadding = (sample['txt_tokens'] != 0).float()
        fn = F.l1_loss if hp['pitch_loss'] == 'l1' else F.mse_loss
        losses['f0'] = _masked_mean(fn(output['pitch_pred'][:, :, 0], sample['f0'], reduction='none'), nonpadding) * hp['lambda_f0']
        return
    mel2ph, f0, uv = sample['mel2ph'], sample['f0'], sample['uv']
    nonpadding = (mel2ph != 0).float()
    if hp['pitch_type'] == 'cwt':
        cwt_pred = output['cwt'][:, :, :10]
        if hp.get('cwt_add_f0_loss') and hp['use_uv']:
            raise ValueError("cwt_add_f0_loss with use_uv: the reference itself fails there - add_f0_loss indexes channel 1 of the one-channel "
                             "f0_cwt_[:, :, None] (tasks/tts/fs2.py:257); set use_uv false to train with the f0 term")
        from . import fs2 as _fs2
        if hp.get('cwt_loss', 'l1') in ('l1', 'l2') and _fs2._CWT_NATIVE['loss'] and _cwt_loss_fusable(output, sample, hp):
            # C / uv / f0_mean / f0_std from one pass over the predictor's output (dsf_cwt_pitch_loss), the gradient of the parent in one more
            t = cwt_pitch_loss_terms(output['cwt'], sample['cwt_spec'], uv if hp['use_uv'] else None, mel2ph, output['f0_mean'], sample['f0_mean'],
                                     output['f0_std'], sample['f0_std'], cwt_loss=hp.get('cwt_loss', 'l1'), use_uv=bool(hp['use_uv']),
                                     lambda_f0=hp['lambda_f0'], lambda_uv=hp['lambda_uv'] if hp['use_uv'] else 0.0)
            losses['C'] = t[0]
            if hp['use_uv']:
                losses['uv'] = t[1]
            losses['f0_mean'], losses['f0_std'] = t[2], t[3]
        else:
            if hp.get('cwt_loss', 'l1') == 'l1':
                c = F.l1_loss(cwt_pred, sample['cwt_spec'])
            elif hp['cwt_loss'] == 'l2':
                c = F.mse_loss(cwt_pred, sample['cwt_spec'])
            elif hp['cwt_loss'] == 'ssim':
                c = mel_loss_terms(cwt_pred, sample['cwt_spec'], bias=20.0, l1=False, ssim=True)[1]
            else:
                raise NotImplementedError(f"cwt_loss {hp['cwt_loss']!r}")
            losses['C'] = c * hp['lambda_f0']
            if hp['use_uv']:
                losses['uv'] = _masked_mean(F.binary_cross_entropy_with_logits(output['cwt'][:, :, -1], uv, reduction='none'), nonpadding) * hp['lambda_uv']
            losses['f0_mean'] = F.l1_loss(output['f0_mean'], sample['f0_mean']) * hp['lambda_f0']
            losses['f0_std'] = F.l1_loss(output['f0_std'], sample['f0_std']) * hp['lambda_f0']
        if hp.get('cwt_add_f0_loss'):
            # tasks/tts/fs2.py:245-247: the f0 the model would synthesise from its own cwt / mean / std (no cwt_std_scale, no frame_keep:
            # the reference calls cwt2f0_norm with its defaults), through add_f0_loss without uv (:254-267)
            from .pe import f0_loss_terms
            f0_cwt = _fs2.cwt2f0_op(cwt_pred, output['f0_mean'], output['f0_std'], mel2ph.shape[1], hp)
            losses['f0'] = f0_loss_terms(f0_cwt[:, :, None], f0, None, nonpadding, use_uv=False, pitch_loss=hp['pitch_loss'], lam_f0=hp['lambda_f0'])[1]
    elif hp['pitch_type'] == 'frame':
        p_pred = output['pitch_pred']
        if hp['use_uv']:
            losses['uv'] = _masked_mean(F.binary_cross_entropy_with_logits(p_pred[:, :, 1], uv, reduction='none'), nonpadding) * hp['lambda_uv']
            nonpadding = nonpadding * (uv == 0).float()
        fn = F.l1_loss if hp['pitch_loss'] == 'l1' else F.mse_loss
        losses['f0'] = _masked_mean(fn(p_pred[:, :, 0], f0, reduction='none'), nonpadding) * hp['lambda_f0']
