"""Developer tool (GPU): the HiFi-GAN mel loss, forward plus backward, at the reference's training shape - 16 x 8192 samples
(configs/tts/hifigan.yaml max_sentences, max_samples), geometry 1024 / 256 / 1024, 80 mel bins - as ONE captured graph of the library path and as
eager calls, beside PyTorch-ROCm eager running the reference's operator sequence (modules/hifigan/mel_utils.py:59-76 with
torch.stft(return_complex=True), l1_loss, autograd) on the same GPU.

    python tools/mel_loss_timing.py [--replays 100] [--out profiles/mel_loss_timing.txt]

HIP events around every replay / eager step, after warm-up; the paths alternate in blocks of 10 so that all see the same machine.  Reported:
median / mean / min of each, the ratio of the medians, the launches of one step of each path with their device time by kernel (torch.profiler;
the library's own launches are 11: 2 x (dsv_mel_spectrum, dsv_mel_head) and 2 of dsf_l1_mean forward, dsf_l1_mean_bwd, dsv_mel_head_backward, 2 of
dsv_stft_adjoint and dsv_mel_clamp_backward backward), and the agreement of the two paths' values.  The shape holds only 32 frames per row: the
result is about launches, not FLOPs."""
import argparse
import datetime
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffsinger_amd import HifiGanMelLoss  # noqa: E402
from tools.stft_loss_timing import device_kernels, kernel_table, timed  # noqa: E402

N_FFT, HOP, WIN, M, SR, FMIN, FMAX = 1024, 256, 1024, 80, 22050, 80, 7600
B, T = 16, 8192


def eager_reference(x, y, basis, window):
    """mel_utils.py:59-76 (return_complex=True) on both waveforms, then F.l1_loss"""
    pad = (N_FFT - HOP) // 2

    def mel(v):
        v = F.pad(torch.clamp(v, -1.0, 1.0).unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
        S = torch.stft(v, N_FFT, hop_length=HOP, win_length=WIN, window=window, center=False, pad_mode='reflect', normalized=False, onesided=True,
                       return_complex=True)
        spec = torch.sqrt(S.real.pow(2) + S.imag.pow(2) + 1e-9)
        return torch.log(torch.clamp(torch.matmul(basis, spec), min=1e-5))
    with torch.no_grad():
        target = mel(y)
    return F.l1_loss(mel(x), target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    assert args.replays >= 50
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(7)
    y = (torch.randn(B, T, generator=g) * 0.1 + 0.3 * torch.sin(torch.arange(T) * 0.05)).to(dev)
    x0 = (y.cpu() + 0.05 * torch.randn(B, T, generator=g)).to(dev)
    crit = HifiGanMelLoss(dict(fft_size=N_FFT, hop_size=HOP, win_size=WIN, audio_num_mel_bins=M, fmin=FMIN, fmax=FMAX, audio_sample_rate=SR)).to(dev)
    basis, window = crit.basis_on(dev), torch.hann_window(WIN, device=dev)

    def lib_step(xg):
        loss = crit(xg, y)
        dx, = torch.autograd.grad(loss, xg)
        return loss.detach(), dx

    def ref_step(xg):
        loss = eager_reference(xg, y, basis, window)
        dx, = torch.autograd.grad(loss, xg)
        return loss.detach(), dx

    static = x0.clone().requires_grad_(True)
    for _ in range(3):                                                       # warm-up: bases, code objects, rocFFT plans
        lib_eager = lib_step(static)
        ref_out = ref_step(static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lib_step(static)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(out, lib_eager)), 'the captured graph does not carry the bits of the eager call'
    t_lib, t_ref, t_lib_eager = [], [], []
    for _ in range(args.replays // 10):
        t_lib += [timed(graph.replay) for _ in range(10)]
        t_ref += [timed(lambda: ref_step(static)) for _ in range(10)]
        t_lib_eager += [timed(lambda: lib_step(static)) for _ in range(10)]
    n_lib, n_ref = device_kernels(lambda: lib_step(static)), device_kernels(lambda: ref_step(static))

    def row(name, ts):
        return f'{name:44s} median {np.median(ts):.4f} ms   mean {np.mean(ts):.4f}   min {np.min(ts):.4f}   ({len(ts)} timed)'

    med_lib, med_ref = float(np.median(t_lib)), float(np.median(t_ref))
    verdict = 'the library path is NOT SLOWER than the eager run' if med_lib <= med_ref else 'the library path IS SLOWER than the eager run: the condition of the issue FAILS'
    lines = [
        f'# {torch.cuda.get_device_name(0)}; HifiGanMelLoss forward + backward (dL/dx), x, y {B} x {T}, geometry {N_FFT} / {HOP} / {WIN}, {M} mel bins',
        f'# HIP events around every replay / step after warm-up, the paths alternating in blocks of 10; torch {torch.__version__}; {datetime.date.today().isoformat()}',
        row('library, one captured graph (replay)', t_lib),
        row('library, eager calls (not captured)', t_lib_eager),
        row('PyTorch-ROCm eager, reference sequence', t_ref),
        f'ratio of the medians, eager reference / captured library: {med_ref / med_lib:.2f} x  ->  {verdict}',
        f'launches of one step: library {sum(n for n, _ in n_lib.values())} (11 of the library; anything else is torch glue); eager reference '
        f'{sum(n for n, _ in n_ref.values())}',
        f'values: library {float(out[0]):.8f}; eager reference {float(ref_out[0]):.8f}; max |dx_lib - dx_ref| {float((out[1] - ref_out[1]).abs().max()):.3e} '
        f'of max |dx| {float(ref_out[1].abs().max()):.3e}',
    ]
    lines += kernel_table('library path by kernel (k_stft<0, 2> spectrum, k_mel_head / k_mel_head_bwd, k_stft<2, 2> adjoint contraction, k_stft_adj_fold the gather)', n_lib)
    lines += kernel_table('eager reference by kernel', n_ref, top=10)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
