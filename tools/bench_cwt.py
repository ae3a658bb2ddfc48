"""Developer tool (GPU): the CWT pitch path (csrc/fs2_cwt.hpp) against the torch expressions it replaces, on the same device and inputs, the two
ways alternating in one process:

  forward    the FastSpeech2 forward of lj_ds_beta6 (pitch_type: cwt, use_uv) at 8 x 1024 frames with the pitch PREDICTED (f0=None: what
             calls cwt2f0_norm; `bench.py --row fs2` is teacher-forced and never does), fs2.set_cwt_native(infer=False / True)
  objective  the cwt terms of the training objective (C, uv, f0_mean, f0_std), forward + backward, on an 8 x 1024 x 11 predictor output,
             fs2.set_cwt_native(loss=False / True); and with cwt_add_f0_loss (use_uv false), which only the operators can compute

    python tools/bench_cwt.py [--iters 50]

Prints one JSON line per measurement: ms (events around `iters` back-to-back evaluations, best of 3 windows) and kernel launches
(torch.profiler) of either way."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffsinger_amd  # noqa: E402
from diffsinger_amd import fs2, hparams, losses  # noqa: E402
from tools.bench_fs2_loss import launches, time_ms  # noqa: E402

DEV = 'cuda:0'


def forward_fn(B=8, T_txt=128, frames_per_phone=8):
    hparams.clear()
    diffsinger_amd.use_preset('lj_ds_beta6')
    torch.manual_seed(1234)
    m = fs2.FastSpeech2(63, 80).to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(7)
    tok = torch.randint(1, 63, (B, T_txt), device=DEV, generator=g)
    T = T_txt * frames_per_phone
    mel2ph = (torch.arange(T, device=DEV) // frames_per_phone + 1)[None].repeat(B, 1)

    @torch.no_grad()
    def run():
        return m(tok, mel2ph=mel2ph, infer=True)['mel_out']
    return run, f'{B}x{T}'


def objective_fn(B=8, T=1024, use_uv=True, add_f0=False):
    g = torch.Generator().manual_seed(11)
    cwt = torch.randn(B, T, 11 if use_uv else 10, generator=g).to(DEV)
    mp, sp = (torch.rand(B, generator=g) + 6.5).to(DEV), (torch.rand(B, generator=g) * 0.5 + 0.2).to(DEV)
    mel2ph = torch.ones(B, T, dtype=torch.int64)
    mel2ph[1:, -100:] = 0
    sample = dict(mel2ph=mel2ph.to(DEV), cwt_spec=torch.randn(B, T, 10, generator=g).to(DEV), uv=(torch.rand(B, T, generator=g) < 0.3).float().to(DEV),
                  f0=(torch.rand(B, T, generator=g) * 2 + 8.5).to(DEV), f0_mean=(torch.rand(B, generator=g) + 6.5).to(DEV),
                  f0_std=(torch.rand(B, generator=g) * 0.5 + 0.2).to(DEV))
    hp = dict(pitch_type='cwt', cwt_loss='l1', use_uv=use_uv, lambda_f0=1.0, lambda_uv=1.0, pitch_loss='l1', pitch_norm='log', cwt_add_f0_loss=add_f0)

    def run():
        out = {'cwt': cwt.detach().requires_grad_(True), 'f0_mean': mp.detach().requires_grad_(True), 'f0_std': sp.detach().requires_grad_(True)}
        L = {}
        losses._add_pitch_loss(out, sample, hp, L)
        total = sum(L.values())
        total.backward()
        return total
    return run, f'{B}x{T}x{cwt.shape[2]}'


def ab(what, shape, fn, key, iters):
    row = {'what': what, 'shape': shape}
    try:
        for rep in range(2):                                     # torch, hip, torch, hip: a drift of the box shows as a difference between the reps
            for on in (False, True):
                fs2.set_cwt_native(**{key: on})
                fn()
                ms = time_ms(fn, iters)
                name = 'hip' if on else 'torch'
                row[f'{name}_ms'] = round(min(ms, row.get(f'{name}_ms', float('inf'))), 4)
                row.setdefault(f'{name}_ms_reps', []).append(round(ms, 4))
                if rep == 0:
                    row[f'{name}_launches'] = launches(fn)
    finally:
        fs2.set_cwt_native(infer=False, loss=True)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    a = ap.parse_args()
    fn, shape = forward_fn()
    ab('FastSpeech2 forward, lj_ds_beta6, pitch predicted (cwt2f0_norm inside)', shape, fn, 'infer', a.iters)
    fn, shape = objective_fn()
    ab('cwt objective (C, uv, f0_mean, f0_std), forward + backward', shape, fn, 'loss', a.iters)
    fn, shape = objective_fn(use_uv=False, add_f0=True)
    fs2.set_cwt_native(loss=True)
    fn()
    print(json.dumps({'what': 'cwt objective with cwt_add_f0_loss (C, f0_mean, f0_std, f0; use_uv false), forward + backward: operators only',
                      'shape': shape, 'hip_ms': round(time_ms(fn, a.iters), 4), 'hip_launches': launches(fn)}), flush=True)


if __name__ == '__main__':
    main()
