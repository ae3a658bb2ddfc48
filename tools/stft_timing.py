"""Developer tool (GPU): HIP-event times of the STFT operators (diffsinger_amd.stft) at the shapes the shipped configs use, beside the wall time
of the host post-filter they replace.  Reported, not gated (profiles/stft_timing.txt, DESIGN.md section "STFT").

    python tools/stft_timing.py [--calls 40] [--out profiles/stft_timing.txt]

Per (n_fft / hop) in 1024 / 256 @ 22 050 Hz and 512 / 128 @ 24 kHz, at 1 x 800 and 8 x 1024 frames: logmel_op ('pwg') and denoise_op, mean / median /
min over `calls` event pairs after 5 warm-up calls.  FLOP of a forward transform = 2 n_fft * 2 n_bins per frame (the accounting of the issue
text, n_bins = n_fft / 2 + 1); denoise_op counts the forward and the inverse product.  Share of peak against 157.3 TFLOP/s (fp32 MFMA)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffsinger_amd import stft as ST                    # noqa: E402
from diffsinger_amd.vocoder import denoise               # noqa: E402

PEAK = 157.3e12


def events(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.mean(ms)), float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    lines = [f'# {torch.cuda.get_device_name(0)}; HIP events, {args.calls} calls after 5 warm-up calls; ms = mean / median / min']
    for n_fft, hop, sr, fmin, fmax in ((1024, 256, 22050, 80, 7600), (512, 128, 24000, 50, 11025)):
        basis = ST.mel_basis_on('cuda:0', sr, n_fft, 80, fmin, fmax)
        for B, T in ((1, 800), (8, 1024)):
            L = T * hop
            g = torch.Generator().manual_seed(B * T)
            wav = (torch.randn(B, L, generator=g) * 0.1 + 0.3 * torch.sin(torch.arange(L) * 0.05)).cuda()
            frames = B * (T + 1)
            flop = 2.0 * n_fft * (n_fft + 2) * frames
            for name, fn, k in (('logmel_op', lambda: ST.logmel_op(wav, basis, n_fft=n_fft, hop=hop, flavour='pwg'), 1),
                                ('denoise_op', lambda: ST.denoise_op(wav, 0.1, fft_size=n_fft, hop_size=hop, win_size=n_fft), 2)):
                mean, med, mn = events(fn, args.calls)
                lines.append(f'{name:10s} n_fft {n_fft} hop {hop}  {B} x {T} frames: {mean:.4f} / {med:.4f} / {mn:.4f} ms; {k * flop / 1e9:.2f} GFLOP '
                             f'-> {k * flop / (mean * 1e-3) / 1e12:.1f} TFLOP/s = {100 * k * flop / (mean * 1e-3) / PEAK:.1f} % of the fp32-MFMA peak (mean)')
            if B == 8:
                # the path this replaces: device -> host copy of the waveform, then the numpy function row by row (HifiGAN.spec2wav handles one utterance)
                t0 = time.perf_counter()
                host = wav.cpu().numpy()
                t1 = time.perf_counter()
                for r in range(B):
                    denoise(host[r], v=0.1, fft_size=n_fft, hop_size=hop, win_size=n_fft)
                t2 = time.perf_counter()
                lines.append(f'host path  n_fft {n_fft} hop {hop}  {B} x {T} frames: device->host copy {1e3 * (t1 - t0):.2f} ms + vocoder.denoise {1e3 * (t2 - t1):.1f} ms '
                             f'(wall, time.perf_counter, one run, same box)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
