"""The FastSpeech2 training objective restated in plain torch (any device, any dtype) - the yardstick of tests/test_gpu_fs2_loss.py.

The reference's task classes do not import without their data / audio stack, so their loss methods are restated here line by line, with the
lines they restate; tests/test_fs2_loss_host.py pins the pieces that do import (modules/commons/ssim.py, mel2ph_to_dur) against this file."""
from math import exp

import torch
import torch.nn.functional as F


def gaussian(window_size=11, sigma=1.5):
    """modules/commons/ssim.py:319-322: exp in double, rounded to fp32 (torch.Tensor), normalised in fp32."""
    g = torch.Tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    return g / g.sum()


def create_window(window_size=11, dtype=torch.float32, device='cpu'):
    """ssim.py:325-329 (one channel), then cast: the window is built in fp32 whatever the dtype of the images."""
    w1 = gaussian(window_size, 1.5).unsqueeze(1)
    return w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).to(dtype=dtype, device=device)


def ssim_map(img1, img2, window_size=11):
    """ssim.py:332-351 (_ssim) without the reduction: the map [B, 1, H, W]."""
    window = create_window(window_size, img1.dtype, img1.device)
    pad = window_size // 2
    mu1 = F.conv2d(img1, window, padding=pad)
    mu2 = F.conv2d(img2, window, padding=pad)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def weights_nonzero_speech(target):
    """tasks/tts/tts.py:124-128"""
    return target.abs().sum(-1, keepdim=True).ne(0).to(target.dtype).repeat(1, 1, target.size(-1))


def l1_loss(mel_out, target):
    """tasks/tts/fs2.py:160-167"""
    w = weights_nonzero_speech(target)
    return (F.l1_loss(mel_out, target, reduction='none') * w).sum() / w.sum()


def ssim_loss(mel_out, target, bias=6.0):
    """tasks/tts/fs2.py:169-178 (ssim(..., size_average=False) = ssim_map.mean(1))"""
    w = weights_nonzero_speech(target)
    s = 1 - ssim_map(mel_out[:, None] + bias, target[:, None] + bias).mean(1)
    return (s * w).sum() / w.sum()


def mel2ph_to_dur(mel2ph, T_txt):
    """modules/fastspeech/tts_modules.py:242-248"""
    B = mel2ph.shape[0]
    return mel2ph.new_zeros(B, T_txt + 1).scatter_add(1, mel2ph, torch.ones_like(mel2ph))[:, 1:]


def dur_loss(dur_pred, mel2ph, txt_tokens, *, sil_ids=None, wdb=None, lam_ph=1.0, lam_word=1.0, lam_sent=1.0):
    """{pdur, wdur, sdur}: FastSpeech2Task.add_dur_loss (tasks/tts/fs2.py:180-219) with sil_ids, the MIDI tasks' add_dur_loss
    (usr/diffsinger_task.py:359-389 = :443-473) with wdb (word_boundary; pdur not scaled: pass lam_ph = 1)."""
    B, T = txt_tokens.shape
    nonpadding = (txt_tokens != 0).to(dur_pred.dtype)
    dur_gt = mel2ph_to_dur(mel2ph, T).to(dur_pred.dtype) * nonpadding
    losses = {}
    pdur = F.mse_loss(dur_pred, (dur_gt + 1).log(), reduction='none')
    losses['pdur'] = (pdur * nonpadding).sum() / nonpadding.sum() * lam_ph
    dur_pred = (dur_pred.exp() - 1).clamp(min=0)
    if wdb is None:
        is_sil = torch.zeros_like(txt_tokens).bool()
        for p in sil_ids:
            is_sil = is_sil | (txt_tokens == p)
        is_sil = is_sil.to(dur_pred.dtype)
        word_id = (is_sil.cumsum(-1) * (1 - is_sil)).long()                                 # :208
        word_dur_p = dur_pred.new_zeros([B, int(word_id.max()) + 1]).scatter_add(1, word_id, dur_pred)[:, 1:]
        word_dur_g = dur_gt.new_zeros([B, int(word_id.max()) + 1]).scatter_add(1, word_id, dur_gt)[:, 1:]
    else:
        idx = F.pad(wdb.cumsum(axis=1), (1, 0))[:, :-1]                                       # usr/diffsinger_task.py:377
        word_dur_p = dur_pred.new_zeros([B, int(idx.max()) + 1]).scatter_add(1, idx, dur_pred)
        word_dur_g = dur_gt.new_zeros([B, int(idx.max()) + 1]).scatter_add(1, idx, dur_gt)
    wdur = F.mse_loss((word_dur_p + 1).log(), (word_dur_g + 1).log(), reduction='none')
    word_nonpadding = (word_dur_g > 0).to(dur_pred.dtype)
    losses['wdur'] = (wdur * word_nonpadding).sum() / word_nonpadding.sum() * lam_word
    sent_dur_p, sent_dur_g = dur_pred.sum(-1), dur_gt.sum(-1)
    losses['sdur'] = F.mse_loss((sent_dur_p + 1).log(), (sent_dur_g + 1).log(), reduction='mean') * lam_sent
    return losses


def mel_case(B, T, M, seed, bias_scale=1.0):
    """mel_out / target [B, T, M] like a decoder's: target rows b > 0 end in zero frames (padding); mel_out zero there too except in the last
    utterance, whose padded frames keep a prediction (the weights must drop it)."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, T, M, generator=g) * 1.2 - 4.0) * bias_scale
    x = y + 0.3 * torch.randn(B, T, M, generator=g) * bias_scale
    for b in range(1, B):
        n = max(1, T // (3 * b + 1))
        if n < T:
            y[b, T - n:] = 0
            if b != B - 1:
                x[b, T - n:] = 0
    return x, y
