"""Developer tool (GPU): one generator step of HiFi-GAN / NSF-HiFi-GAN training - HifiGanGenerator.forward_train + MSE + backward to every
parameter - at the batch shape of configs/tts/hifigan.yaml (16 x 8192 samples, c0 = 128, rates [8, 8, 2, 2], NSF), timed with device events:

    hip eager     diffsinger_amd.HifiGanGenerator.forward_train, call by call            (--mode eager)
    hip graph     the same step captured once on ONE stream and replayed                 (--mode graph)
    torch eager   the same operator sequence on PyTorch-ROCm: tests/hifigan_train_helpers.generator in float32 with autograd

The torch variant runs in its OWN CHILD PROCESS (this file again with --child): no process holds this library's training path and torch's
eager device convolutions at once.  Both processes build the same seeded state and inputs on the host.  Every window holds at least
--min-seconds of device time; the figure of a variant is the median over its windows.  Per tensor, each variant's gradients are compared with
float64 (the helpers' restatement on the CPU) on that variant's OWN leaky-ReLU masks and sine_waves: max |grad - grad64| / max |grad64|.

    python tools/hifigan_gen_timing.py [--batch 16] [--samples 8192] [--mode eager|graph] [--out profiles/hifigan_gen_timing.txt]
    python tools/hifigan_gen_timing.py --profile-loop 5      # nothing but 5 eager HIP steps (for rocprofv3 --kernel-trace --stats -- python ...)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import hifigan_train_helpers as TH  # noqa: E402

H_TRAIN = dict(resblock='1', upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=128,
               resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, audio_sample_rate=24000)


def problem(args):
    """the seeded state and inputs, identical in both processes (host tensors)"""
    h = dict(H_TRAIN, use_pitch_embed=not args.plain)
    hop = TH.hop_of(h)
    assert args.samples % hop == 0
    B, T = args.batch, args.samples // hop
    state = TH.synth_state(TH.module_shapes(h), 7)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(B, 80, T, generator=gen)
    target = 0.3 * torch.randn(B, 1, args.samples, generator=gen)
    f0 = None
    if not args.plain:
        f0 = 180.0 + 120.0 * torch.rand(B, T, generator=gen)
        f0[:, T // 3:T // 3 + max(1, T // 8)] = 0.0
    draws = (torch.rand(B, 9, generator=gen), torch.randn(B, args.samples, 9, generator=gen))
    return h, state, x, f0, target, draws


def window(fn, min_s):
    """run fn repeatedly until the window holds at least min_s of device time -> ms per call"""
    n, total, calls = 1, 0.0, 0
    while total < min_s * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        calls += n
        n *= 2
    return total / calls


def against_float64(h, state, x, f0, target, grads, pre, sw):
    """per tensor max |grad - grad64| / max |grad64| against the float64 restatement on the CPU on THESE masks and sine_waves -> sorted rows"""
    masks = TH.masks_of(pre)
    _, g64, _, _, _ = TH.module_grads(state, h, x, f0, TH.mse_to(target), masks=masks, sine_waves=None if sw is None else sw.detach().cpu())
    rows = sorted(((float((TH.d64(grads[k]) - g64[k]).abs().max() / g64[k].abs().max()), k) for k in g64 if g64[k] is not None), reverse=True)
    return rows


def child(args):
    """torch eager: the helpers' restatement in float32 on the device with autograd -> one JSON line"""
    from oracle import hifigan_oracle as O
    h, state, x, f0, target, _ = problem(args)
    dev = 'cuda'
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in state.items()}
    xd, td = x.to(dev), target.to(dev)
    sw = None
    if f0 is not None:
        torch.manual_seed(9)
        f0u = F.interpolate(f0[:, None], scale_factor=float(TH.hop_of(h)), mode='nearest').transpose(1, 2)
        sw = O.sine_gen(f0u, h['audio_sample_rate'])[0].to(dev)
    f0d = None if f0 is None else f0.to(dev)
    keys = list(leaves)

    def step(want_pre=False):
        out, pre, _, _ = TH.generator(TH.plain_weights(leaves, h), h, xd, f0d, sine_waves=sw)
        gs = torch.autograd.grad(torch.mean((out - td) ** 2), [leaves[k] for k in keys])
        return (gs, pre) if want_pre else gs
    rows = []
    if not args.no_accuracy:
        gs, pre = step(True)
        rows = against_float64(h, state, x, f0, target, dict(zip(keys, gs)), [p.detach() for p in pre], sw)
        del gs, pre
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    times = [window(step, args.min_seconds) for _ in range(args.windows)]
    print('CHILD ' + json.dumps(dict(times=times, worst=rows[:6], peak=torch.cuda.max_memory_allocated() / 2 ** 30)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hifigan_gen_timing.txt'))
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--samples', type=int, default=8192)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--mode', choices=['eager', 'graph'], default='eager')
    ap.add_argument('--plain', action='store_true', help='without the NSF source')
    ap.add_argument('--no-torch', action='store_true', help='skip the torch eager child process')
    ap.add_argument('--no-accuracy', action='store_true', help='skip the float64 comparison on the CPU')
    ap.add_argument('--profile-loop', type=int, default=0)
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hifigan_gen_timing: needs the GPU (a timing taken anywhere else says nothing)')
    if args.child:
        return child(args)
    from diffsinger_amd.build import binary_id
    from diffsinger_amd.vocoder import HifiGanGenerator
    dev = 'cuda'
    h, state, x, f0, target, draws = problem(args)
    m = HifiGanGenerator(h)
    m.load_state_dict(state, strict=True)
    m = m.to(dev)
    xd, td = x.to(dev), target.to(dev)
    f0d = None if f0 is None else f0.to(dev)
    kw = {} if f0 is None else dict(rand_ini=draws[0].to(dev), noise=draws[1].to(dev))
    names, params = zip(*m.named_parameters())

    def hip_step():
        y = m.forward_train(xd, f0d, **kw)
        return torch.autograd.grad(torch.mean((y - td) ** 2), params)

    if args.profile_loop:
        for _ in range(args.profile_loop):
            hip_step()
        torch.cuda.synchronize()
        return
    lines = [f'HiFi-GAN generator step (forward_train + MSE + backward to every parameter), B x samples = {args.batch} x {args.samples}, '
             f'c0 = {h["upsample_initial_channel"]}, rates {h["upsample_rates"]}, {"NSF" if f0 is not None else "plain"}; hip mode: {args.mode}',
             f'device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library build {binary_id()[:16]}',
             f'{args.windows} windows of >= {args.min_seconds} s device time per variant, device events; median (min .. max) ms per step']
    s = torch.cuda.Stream()                                          # ONE stream for everything this process enqueues
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip_step()
        s.synchronize()
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        with torch.no_grad():
            t_fwd = [window(lambda: m(xd, f0d, **kw), args.min_seconds) for _ in range(3)]
            t_fwt = [window(lambda: m.forward_train(xd, f0d, **kw), args.min_seconds) for _ in range(3)]       # the node's forward alone
        if not args.no_accuracy:
            y, pre, sw = m.forward_train(xd, f0d, return_saved=True, **kw)
            gs = torch.autograd.grad(torch.mean((y - td) ** 2), params)
            with torch.no_grad():
                same = torch.equal(m(xd, f0d, **kw), y)
            rows = against_float64(h, state, x, f0, target, dict(zip(names, gs)), pre, sw)
            lines.append(f'forward_train bitwise equal to forward(): {same}; hip gradients against float64 on their own masks, per tensor max |grad - grad64| / '
                         f'max |grad64|, the six largest: ' + ', '.join(f'{k} {e:.2e}' for e, k in rows[:6]))
            del y, pre, sw, gs
        fn = hip_step
        if args.mode == 'graph':
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                hip_step()
            fn = graph.replay
        for _ in range(3):
            fn()
        s.synchronize()
        t_hip = [window(fn, args.min_seconds) for _ in range(args.windows)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    med = statistics.median(t_hip)
    mf, mt = statistics.median(t_fwd), statistics.median(t_fwt)
    lines.append(f'  hip {args.mode:6s} {med:8.3f}  ({min(t_hip):.3f} .. {max(t_hip):.3f});  forward() alone (fused chains, cached packed weights) {mf:.3f} ms, '
                 f'the training forward alone (one launch per convolution, weights packed per call, eager) {mt:.3f} ms = {mt / mf:.1f} x; the training step '
                 f'is {med / mf:.1f} x the inference forward; peak device memory of one eager hip step {peak:.2f} GiB')
    if not args.no_torch:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--batch', str(args.batch), '--samples', str(args.samples), '--windows', str(args.windows),
               '--min-seconds', str(args.min_seconds)] + (['--plain'] if args.plain else []) + (['--no-accuracy'] if args.no_accuracy else [])
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith('CHILD ')]
        if out.returncode != 0 or not got:
            raise SystemExit(f'hifigan_gen_timing: the torch eager child process failed ({out.returncode}):\n{out.stderr[-2000:]}')
        js = json.loads(got[-1][6:])
        tm = statistics.median(js['times'])
        lines.append(f'  torch eager {tm:8.3f}  ({min(js["times"]):.3f} .. {max(js["times"]):.3f})  (its own process; peak device memory {js["peak"]:.2f} GiB)')
        if js['worst']:
            lines.append('torch eager gradients against float64 on their own masks, the six largest: ' + ', '.join(f'{k} {e:.2e}' for e, k in js['worst']))
        lines.append(f'hip {args.mode} / torch eager = {med / tm:.3f}')
        if med > tm:
            lines.append('THE HIP PATH IS SLOWER THAN TORCH EAGER at this shape (see the kernel trace for the kernels that cost it)')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n\n')


if __name__ == '__main__':
    main()
