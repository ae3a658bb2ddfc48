"""Developer tool (GPU): one training-side step of the ParallelWaveGAN discriminator - forward + generator_loss + backward with respect to the
input and every parameter - at the batch shape of configs/tts/pwg.yaml (max_sentences 5 x max_samples 25600), timed with device events:

    hip eager     diffsinger_amd.ParallelWaveGANDiscriminator, call by call
    hip graph     the same step captured once into a torch.cuda.graph and replayed
    torch eager   the reference module's operator sequence on PyTorch-ROCm: a Conv1d / LeakyReLU(inplace) stack with weight norm built HERE
                  (same shapes and dilations as modules/parallel_wavegan/models/parallel_wavegan.py:207-300), loss by torch.mean

All three in one process, alternating, warmed, every window at least 0.5 s of device time; the figure of a variant is the median over its windows.
Bounds derived from the shapes (not measured): 75 GFLOP of fp32 MFMA work = 0.48 ms at 157 TF, 1.8 GB of traffic = 0.29 ms at 6.3 TB/s.

    python tools/pwg_disc_timing.py [--out profiles/pwg_disc_timing.txt] [--windows 5] [--batch 5] [--samples 25600]
    python tools/pwg_disc_timing.py --profile-loop 20       # nothing but 20 eager HIP steps (for rocprofv3 --kernel-trace --stats -- python ...)"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_BOUND_MS, HBM_BOUND_MS = 0.48, 0.29


def torch_stack(layers=10, channels=64, slope=0.2):
    mods, ci = [], 1
    for i in range(layers - 1):
        d = 1 if i == 0 else i
        mods += [nn.utils.weight_norm(nn.Conv1d(ci, channels, 3, padding=d, dilation=d)), nn.LeakyReLU(slope, inplace=True)]
        ci = channels
    mods.append(nn.utils.weight_norm(nn.Conv1d(ci, 1, 3, padding=1)))
    return nn.Sequential(*mods)


def window(fn, min_s):
    """run fn repeatedly until the window holds at least min_s of device time -> ms per call"""
    n, total = 4, 0.0
    calls = 0
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pwg_disc_timing.txt'))
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--samples', type=int, default=25600)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--profile-loop', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pwg_disc_timing: needs the GPU (a timing taken anywhere else says nothing)')
    import warnings
    warnings.filterwarnings('ignore', category=FutureWarning)
    from diffsinger_amd import ParallelWaveGANDiscriminator, generator_loss
    from diffsinger_amd import pwg_disc as PD
    from diffsinger_amd.build import binary_id
    dev = 'cuda'
    torch.manual_seed(0)
    hip = ParallelWaveGANDiscriminator().to(dev)
    ref = torch_stack().to(dev)
    with torch.no_grad():                                        # the same O(1) parameters in both
        for i in range(10):
            c, r = hip.conv_layers[2 * i], ref[2 * i]
            r.weight_v.normal_()
            r.weight_g.fill_(1.35)
            r.bias.normal_(0, 0.1)
            c.weight_v.copy_(r.weight_v); c.weight_g.copy_(r.weight_g); c.bias.copy_(r.bias)
    x = torch.randn(args.batch, 1, args.samples, device=dev).requires_grad_(True)
    hp, rp = list(hip.parameters()), list(ref.parameters())

    def hip_step():
        return torch.autograd.grad(generator_loss([hip(x)]), [x] + hp)

    def ref_step():
        return torch.autograd.grad(torch.mean((1 - ref(x)) ** 2), [x] + rp)

    if args.profile_loop:
        for _ in range(args.profile_loop):
            hip_step()
        torch.cuda.synchronize()
        return
    n0 = PD.launch_count()
    gh = hip_step()
    launches = PD.launch_count() - n0
    gr = ref_step()
    dx_rel = float((gh[0] - gr[0]).abs().max() / gr[0].abs().max())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_step()
    variants = [('hip eager', hip_step), ('hip graph', graph.replay), ('torch eager', ref_step)]
    for _, fn in variants:                                       # warm every variant
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(args.windows):
        for name, fn in variants:                                # alternating
            times[name].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f'ParallelWaveGAN discriminator step (forward + generator_loss + backward, dx and all parameter gradients), B x T = {args.batch} x {args.samples}',
             f'device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library build {binary_id()[:16]}',
             f'{args.windows} alternating windows of >= {args.min_seconds} s device time per variant, device events; median (min .. max) ms per step',
             f'library launches per hip step: {launches} (torch glue - weight norm and its gradient, stacking the matrices - not counted)',
             f'max |dx_hip - dx_torch| / max |dx_torch| = {dx_rel:.2e} (float32 sign flips of near-zero pre-activations included)']
    for name, _ in variants:
        v = times[name]
        lines.append(f'  {name:12s} {med[name]:8.3f}  ({min(v):.3f} .. {max(v):.3f})')
    lines.append(f'hip eager / torch eager = {med["hip eager"] / med["torch eager"]:.3f}   hip graph / torch eager = {med["hip graph"] / med["torch eager"]:.3f}')
    for name in ('hip eager', 'hip graph'):
        lines.append(f'{name}: MFMA bound {MFMA_BOUND_MS} ms is {100 * MFMA_BOUND_MS / med[name]:.1f} % of the step, HBM bound {HBM_BOUND_MS} ms {100 * HBM_BOUND_MS / med[name]:.1f} %')
    if med['hip graph'] > med['torch eager']:
        lines.append('THE HIP PATH IS SLOWER THAN TORCH EAGER at this shape (see the kernel trace for the kernel that costs it)')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
