"""Developer tool (GPU): the multi-resolution STFT loss, forward plus backward, at the reference's training shape - 5 x 25600 samples
(configs/tts/pwg.yaml:13-14 batch_max_steps, batch_size; the three resolutions of :77-82) - as ONE captured graph of the library path, beside
PyTorch-ROCm eager running the reference's operator sequence (torch.stft(return_complex=True) + autograd) on the same GPU.

    python tools/stft_loss_timing.py [--replays 100] [--out profiles/stft_loss_timing.txt]

HIP events around every replay / eager step, after warm-up; the two paths alternate in blocks of 10 so that both see the same machine.
Reported: median / mean / min of each, the ratio of the medians, the launches of one step of each path with their device time by kernel (torch.profiler; the library's own
launches are 7 per resolution: 2 dsv_stft, 2 dsv_spectral_loss, 1 dsv_spectral_loss_backward, 2 dsv_stft_adjoint), and the agreement of the
two paths' values."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffsinger_amd import MultiResolutionSTFTLoss  # noqa: E402

RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
B, T = 5, 25600


def eager_reference(x, y, windows):
    """modules/parallel_wavegan/losses/stft_loss.py:12-153 with return_complex=True"""
    sc = mag = 0.0
    for (n_fft, hop, win), w in zip(RES, windows):
        mags = []
        for s in (x, y):
            S = torch.stft(s, n_fft, hop, win, w, return_complex=True)
            mags.append(torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-7)).transpose(2, 1))
        xm, ym = mags
        sc = sc + torch.norm(ym - xm, p='fro') / torch.norm(ym, p='fro')
        mag = mag + torch.nn.functional.l1_loss(torch.log(ym), torch.log(xm))
    return sc / len(RES), mag / len(RES)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def device_kernels(fn):
    """{kernel name: (launches, device microseconds)} of one call, by torch.profiler (copies and memsets left out)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'emcpy' not in e.name and 'emset' not in e.name:
            n, us = out.get(e.name, (0, 0.0))
            out[e.name] = (n + 1, us + float(e.time_range.elapsed_us()))
    assert out, 'torch.profiler recorded no device kernel: the launch count cannot be stated'
    return out


def kernel_table(title, k, top=None):
    rows = sorted(k.items(), key=lambda kv: -kv[1][1])
    lines = [f'{title}: {sum(n for n, _ in k.values())} device kernels, {sum(us for _, us in k.values()) / 1e3:.3f} ms of kernel time in one profiled eager step']
    for name, (n, us) in rows[:top]:
        lines.append(f'    {n:3d} x {us / 1e3:8.4f} ms  {name[:110]}')
    if top is not None and len(rows) > top:
        lines.append(f'    ... {len(rows) - top} more kernel names, {sum(us for _, (_, us) in rows[top:]) / 1e3:.4f} ms')
    return lines


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
    crit = MultiResolutionSTFTLoss()
    windows = [torch.hann_window(win, device=dev) for _, _, win in RES]

    def lib_step(xg):
        sc, mag = crit(xg, y)
        dx, = torch.autograd.grad(sc + mag, xg)
        return sc.detach(), mag.detach(), dx

    def ref_step(xg):
        sc, mag = eager_reference(xg, y, windows)
        dx, = torch.autograd.grad(sc + mag, xg)
        return sc.detach(), mag.detach(), dx

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

    def row(name, ts, extra=''):
        return f'{name:44s} median {np.median(ts):.4f} ms   mean {np.mean(ts):.4f}   min {np.min(ts):.4f}   ({len(ts)} timed){extra}'

    med_lib, med_ref = float(np.median(t_lib)), float(np.median(t_ref))
    verdict = 'the library path is NOT SLOWER than the eager run' if med_lib <= med_ref else 'the library path IS SLOWER than the eager run: the condition of the issue FAILS'
    lines = [
        f'# {torch.cuda.get_device_name(0)}; MultiResolutionSTFTLoss forward + backward (d(sc + mag)/dx), x, y {B} x {T}, resolutions {RES}',
        f'# HIP events around every replay / step after warm-up, the paths alternating in blocks of 10; torch {torch.__version__}',
        row('library, one captured graph (replay)', t_lib),
        row('library, eager calls (not captured)', t_lib_eager),
        row('PyTorch-ROCm eager, torch.stft + autograd', t_ref),
        f'ratio of the medians, eager reference / captured library: {med_ref / med_lib:.2f} x  ->  {verdict}',
        f'launches of one step: library {sum(n for n, _ in n_lib.values())} (21 of the library - 7 per resolution - the rest torch glue: the mean over resolutions, its '
        f'backward, the accumulation of dx); eager reference {sum(n for n, _ in n_ref.values())}',
        f'values: library sc {float(out[0]):.8f} mag {float(out[1]):.8f}; eager reference sc {float(ref_out[0]):.8f} mag {float(ref_out[1]):.8f}; '
        f'max |dx_lib - dx_ref| {float((out[2] - ref_out[2]).abs().max()):.3e} of max |dx| {float(ref_out[2].abs().max()):.3e}',
    ]
    lines += kernel_table('library path by kernel (k_stft<0, 2> forward, k_stft<2, 2> adjoint contraction, k_stft_adj_fold the gather)', n_lib)
    lines += kernel_table('eager reference by kernel', n_ref, top=8)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
