"""Developer tool (GPU): the FastSpeech2 training objective - mel L1 + SSIM and the duration terms, forward + backward - the reference's torch way
(tests/fs2_loss_helpers.py: five 11 x 11 conv2d on the GPU's vendor convolutions, the element-wise chain, scatter_add sized by the data) against
the HIP kernels (diffsinger_amd/losses.py), on the same device and inputs.

    python tools/bench_fs2_loss.py [--shapes 8x1024,1x800] [--iters 50]

Prints one JSON line per shape: ms per objective (events around `iters` back-to-back evaluations, best of 3 windows) and kernel launches per
objective (torch.profiler), both ways."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsinger_amd import losses  # noqa: E402
from tests import fs2_loss_helpers as LH  # noqa: E402

SIL = [1, 2, 5, 9]


def inputs(B, T, dev):
    x, y = LH.mel_case(B, T, 80, seed=B * 7 + T)
    g = torch.Generator().manual_seed(T)
    Tt = max(8, T // 6)
    tok = torch.randint(3, 60, (B, Tt), generator=g)
    tok[:, ::7] = 1
    dur = torch.full((B, Tt), T // Tt)
    mel2ph = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        ids = torch.repeat_interleave(torch.arange(1, Tt + 1), dur[b])[:T]
        mel2ph[b, :ids.numel()] = ids
    dp = torch.randn(B, Tt, generator=g) * 0.5 + 1.5
    return x.to(dev), y.to(dev), dp.to(dev), mel2ph.to(dev), tok.to(dev)


def torch_way(x, y, dp, mel2ph, tok):
    xr, dr = x.detach().requires_grad_(True), dp.detach().requires_grad_(True)
    L = LH.dur_loss(dr, mel2ph, tok, sil_ids=SIL)
    loss = 0.5 * LH.l1_loss(xr, y) + 0.5 * LH.ssim_loss(xr, y) + sum(L.values())
    loss.backward()
    return loss


def hip_way(x, y, dp, mel2ph, tok, sil):
    xr, dr = x.detach().requires_grad_(True), dp.detach().requires_grad_(True)
    t = losses.mel_loss_terms(xr, y, lam_l1=0.5, lam_ssim=0.5)
    d = losses.dur_loss_terms(dr, mel2ph, tok, sil_ids=sil)
    loss = t[0] + t[1] + d.sum()
    loss.backward()
    return loss


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type.name == 'CUDA' and 'Memcpy' not in e.name and 'Memset' not in e.name)
    except Exception as e:                      # the profiler is optional here
        return f'n/a ({type(e).__name__})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x1024,1x800')
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    dev = 'cuda:0'
    sil = torch.tensor(SIL, device=dev)
    for s in a.shapes.split(','):
        B, T = (int(v) for v in s.split('x'))
        args = inputs(B, T, dev)
        lt, lh = float(torch_way(*args)), float(hip_way(*args, sil))
        row = {'shape': f'{B}x{T}x80', 'objective': 'mel l1 + ssim + pdur / wdur / sdur, forward + backward',
               'torch_ms': round(time_ms(lambda: torch_way(*args), a.iters), 4), 'hip_ms': round(time_ms(lambda: hip_way(*args, sil), a.iters), 4),
               'torch_launches': launches(lambda: torch_way(*args)), 'hip_launches': launches(lambda: hip_way(*args, sil)),
               'loss_torch': lt, 'loss_hip': lh}
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
