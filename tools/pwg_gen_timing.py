"""Developer tool (GPU): one generator step of the ParallelWaveGAN trainer - forward_train + pwg_generator_losses (multi-resolution STFT loss and
the adversarial term, lambda_adv 4) + backward to every generator parameter - at the batch shape of configs/tts/pwg.yaml (max_sentences 5 x
max_samples 25600), timed with device events:

    hip eager     diffsinger_amd.ParallelWaveGANGenerator.forward_train, call by call
    hip graph     the same step captured once into a torch.cuda.graph and replayed
    torch eager   the reference generator's operator sequence on PyTorch-ROCm: weight-normed Conv1d / gated residual stack / stretch + Conv2d
                  upsampling built HERE from torch modules (the shapes of modules/parallel_wavegan/models/parallel_wavegan.py:21-177), under
                  the SAME objective operators (this package's STFT loss and discriminator) - the two variants differ in the generator only

All in one process on the same inputs and parameters, alternating, warmed, every window at least 0.5 s of device time; the figure of a variant is
the median over its windows.  Bounds derived from the shapes (not measured) are printed beside the times: the generator's fp32 MFMA work
(forward 2 x 128 x (192 + aux + 64) per sample and block, backward twice that) at 157 TF and the traffic of the saved state (x_l and a_l written
once, read by the backward) at 6.3 TB/s.

    python tools/pwg_gen_timing.py [--out profiles/pwg_gen_timing.txt] [--windows 5] [--batch 5] [--samples 25600]
    python tools/pwg_gen_timing.py --profile-loop 5        # nothing but 5 eager HIP steps (for rocprofv3 --kernel-trace --stats -- python ...)"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS, STACKS, AUX, CTX, SCALES = 30, 3, 80, 2, (4, 4, 4, 4)


class TorchBlock(nn.Module):
    def __init__(self, dil):
        super().__init__()
        wn = nn.utils.weight_norm
        self.conv = wn(nn.Conv1d(64, 128, 3, padding=dil, dilation=dil))
        self.conv1x1_aux = wn(nn.Conv1d(AUX, 128, 1, bias=False))
        self.conv1x1_out = wn(nn.Conv1d(64, 64, 1))
        self.conv1x1_skip = wn(nn.Conv1d(64, 64, 1))

    def forward(self, x, c):
        a = self.conv(x) + self.conv1x1_aux(c)
        z = torch.tanh(a[:, :64]) * torch.sigmoid(a[:, 64:])
        return (self.conv1x1_out(z) + x) * math.sqrt(0.5), self.conv1x1_skip(z)


class TorchGenerator(nn.Module):
    def __init__(self):
        super().__init__()
        wn = nn.utils.weight_norm
        self.first_conv = wn(nn.Conv1d(1, 64, 1))
        self.conv_in = wn(nn.Conv1d(AUX, AUX, 2 * CTX + 1, bias=False))
        self.up = nn.ModuleList([wn(nn.Conv2d(1, 1, (1, 2 * s + 1), padding=(0, s), bias=False)) for s in SCALES])
        self.conv_layers = nn.ModuleList([TorchBlock(2 ** (i % (LAYERS // STACKS))) for i in range(LAYERS)])
        self.last1, self.last3 = wn(nn.Conv1d(64, 64, 1)), wn(nn.Conv1d(64, 1, 1))

    def forward(self, x, c, masks=None, want_saved=False):
        """masks = (m1, m2): the two ReLUs of the output layers as products with GIVEN 0 / 1 masks instead of their own sign tests"""
        c = self.conv_in(c).unsqueeze(1)
        for s, f in zip(SCALES, self.up):
            c = f(F.interpolate(c, scale_factor=(1, s), mode='nearest'))
        c = c.squeeze(1)
        x = self.first_conv(x)
        skips = 0
        for blk in self.conv_layers:
            x, h = blk(x, c)
            skips = skips + h
        skips = skips * math.sqrt(1.0 / LAYERS)
        m1 = (skips > 0) if masks is None else masks[0]
        o1 = self.last1(skips * m1.to(skips.dtype))
        m2 = (o1 > 0) if masks is None else masks[1]
        out = self.last3(o1 * m2.to(o1.dtype))
        return (out, skips.detach(), o1.detach()) if want_saved else out


def pairs(hip, ref):
    """(hip parameter holder, torch module) in one order"""
    out = [(hip.first_conv, ref.first_conv), (hip.upsample_net.conv_in, ref.conv_in)]
    out += [(hip.upsample_net.upsample.up_layers[2 * i + 1], ref.up[i]) for i in range(len(SCALES))]
    for hb, rb in zip(hip.conv_layers, ref.conv_layers):
        out += [(hb.conv, rb.conv), (hb.conv1x1_aux, rb.conv1x1_aux), (hb.conv1x1_out, rb.conv1x1_out), (hb.conv1x1_skip, rb.conv1x1_skip)]
    return out + [(hip.last_conv_layers[1], ref.last1), (hip.last_conv_layers[3], ref.last3)]


# Both variants are float32 evaluations of one objective through 30 gated blocks and two ReLUs.  Each is judged against float64 (ACCURATE below);
# between themselves they differ by the ReLU inputs that their forwards put on different sides of zero - one such element of 16 million moves
# every upstream gradient by the order of 1e-3 of its max-abs at this shape.  The direct comparison is printed with the tensors beyond AGREE
# marked; it is the float64 comparison on each variant's own masks that decides whether a ratio is reported.
AGREE = 1e-2
# Against float64 on the variant's own ReLU masks only float32 arithmetic is left: 30 blocks of k-ordered sums, about 1e-6 of a tensor's max-abs.
ACCURATE = 1e-4


def compare_gradients(names, gh, gr, first_conv):
    """-> (report lines, names that disagree).  first_conv.weight_v has one element per row: its gradient is mathematically zero and both sides
    hold rounding noise of the weight-norm expression; it is judged on its own scale, max |d weight_g| * max |g| / min |v| (the size of the
    two terms that cancel), with the limit 1e-4 on either side."""
    rows, bad = [], []
    for n, a, b in zip(names, gh, gr):
        b = b.reshape(a.shape)
        if n == 'first_conv.weight_v':
            continue
        rows.append((float((a - b).abs().max() / b.abs().max()), n, float(b.abs().max())))
    rows.sort(reverse=True)
    lines = [f'    {n:48s} {r:.2e}  (max |grad_torch| {m:.2e})' + ('' if r <= AGREE else '  BEYOND ' + format(AGREE, 'g')) for r, n, m in rows[:8]]
    i = names.index('first_conv.weight_v')
    scale = float(gr[i - 1].abs().max() * first_conv.weight_g.detach().abs().max() / first_conv.weight_v.detach().abs().min())
    zh, zr = float(gh[i].abs().max()) / scale, float(gr[i].abs().max()) / scale
    lines.append(f'    first_conv.weight_v (mathematically zero): max |grad| over the scale of its cancelling terms: hip {zh:.1e}, torch {zr:.1e} (limit 1e-4)')
    if not (zh <= 1e-4 and zr <= 1e-4):
        bad.append('first_conv.weight_v')
    return lines, bad


def ref_modules(ref):
    """the torch generator's parameter holders in the order of pairs()"""
    out = [ref.first_conv, ref.conv_in] + list(ref.up)
    for rb in ref.conv_layers:
        out += [rb.conv, rb.conv1x1_aux, rb.conv1x1_out, rb.conv1x1_skip]
    return out + [ref.last1, ref.last3]


def ref_params(ref):
    """weight_g, weight_v(, bias) of every holder but the last block's conv1x1_out"""
    out = []
    for m in ref_modules(ref):
        if m is not ref.conv_layers[LAYERS - 1].conv1x1_out:
            out += [m.weight_g, m.weight_v] + ([m.bias] if m.bias is not None else [])
    return out


def against_float64(names, hip, ref, hp, rp, x, c, g):
    """Which variant is the accurate one, at the timed shape.  The SAME upstream gradient g = dL/dy (taken once from the hip variant's objective)
    is sent back through the hip generator, the torch float32 generator and a float64 copy of the torch generator (torch's native kernels on the
    device); per tensor max |grad - grad64| / max |grad64|.  The gradient of a ReLU network is DISCONTINUOUS where a pre-activation lies within
    the forward's rounding error of zero: a float32 forward that puts one such element on the other side of zero than float64 does has a
    different, equally valid, gradient - by |w g| of that element in everything upstream.  So each variant is compared twice: with the float64
    pass using its own sign tests, and with the float64 pass using the MASKS OF THAT VARIANT'S float32 forward (the gradient of the function the
    variant actually evaluated).  The second figure is the arithmetic error of the backward; the difference between the two is mask flips.
    -> (report lines, worst second figure of hip, of torch)"""
    ref64 = TorchGenerator().to(x.device).double()
    ref64.load_state_dict(ref.state_dict())
    p64 = ref_params(ref64)
    yh, (Sh, o1h) = hip.forward_train(x, c, return_saved=True)
    gh = torch.autograd.grad((yh * g).sum(), hp)
    yr, Sr, o1r = ref(x, c, want_saved=True)
    gr = torch.autograd.grad((yr * g).sum(), rp)
    x64, c64, gd = x.double(), c.double(), g.double()
    with torch.backends.cudnn.flags(enabled=False):
        y64, S64, o164 = ref64(x64, c64, want_saved=True)
        g64 = torch.autograd.grad((y64 * gd).sum(), p64)
        del y64
        g64h = torch.autograd.grad((ref64(x64, c64, masks=(Sh > 0, o1h > 0)) * gd).sum(), p64)
        g64r = torch.autograd.grad((ref64(x64, c64, masks=(Sr > 0, o1r > 0)) * gd).sum(), p64)

    def worst(gs, want):
        return max((float((a.double().reshape(b.shape) - b).abs().max() / b.abs().max()), n) for n, a, b in zip(names, gs, want)
                   if n != 'first_conv.weight_v')
    lines, second = [], []
    for label, gs, own, S_, o1_ in (('hip', gh, g64h, Sh, o1h), ('torch float32', gr, g64r, Sr, o1r)):
        flips = int(((S_ > 0) != (S64 > 0)).sum()) + int(((o1_ > 0) != (o164 > 0)).sum())
        (e1, n1), (e2, n2) = worst(gs, g64), worst(gs, own)
        second.append(e2)
        lines.append(f'    {label:14s} float64 with its own sign tests: worst {e1:.2e} ({n1});  float64 with this variant\'s ReLU masks: worst {e2:.2e} '
                     f'({n2});  ReLU inputs on the other side of zero than in float64: {flips} of {S_.numel() + o1_.numel()}')
    return lines, second[0], second[1]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pwg_gen_timing.txt'))
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--samples', type=int, default=25600)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--profile-loop', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pwg_gen_timing: needs the GPU (a timing taken anywhere else says nothing)')
    import warnings
    warnings.filterwarnings('ignore', category=FutureWarning)
    from diffsinger_amd import MultiResolutionSTFTLoss, ParallelWaveGANDiscriminator, generator_loss, pwg_generator_losses
    from diffsinger_amd import pwg_train as PT
    from diffsinger_amd.build import binary_id
    from diffsinger_amd.pwg import ParallelWaveGANGenerator
    dev = 'cuda'
    torch.manual_seed(0)
    hop = int(math.prod(SCALES))
    B, T = args.batch, args.samples
    assert T % hop == 0
    hip = ParallelWaveGANGenerator(layers=LAYERS, stacks=STACKS, aux_channels=AUX, aux_context_window=CTX,
                                   upsample_params={'upsample_scales': list(SCALES)}).to(dev)
    ref = TorchGenerator().to(dev)
    disc = ParallelWaveGANDiscriminator().to(dev)
    stft = MultiResolutionSTFTLoss().to(dev)
    with torch.no_grad():                                        # the same O(1) parameters in both generators
        for h, r in pairs(hip, ref):
            fan_in = r.weight_v[0].numel()
            r.weight_v.normal_(0, fan_in ** -0.5)
            r.weight_g.uniform_(0.7, 1.3)
            h.weight_v.copy_(r.weight_v.reshape(h.weight_v.shape)); h.weight_g.copy_(r.weight_g.reshape(h.weight_g.shape))
            if r.bias is not None:
                r.bias.normal_(0, 0.1)
                h.bias.copy_(r.bias)
        for i in range(10):
            m = disc.conv_layers[2 * i]
            m.weight_v.normal_(); m.weight_g.fill_(1.35); m.bias.normal_(0, 0.1)
    x, c = torch.randn(B, 1, T, device=dev), torch.randn(B, AUX, T // hop + 2 * CTX, device=dev)
    y = 0.3 * torch.randn(B, 1, T, device=dev)
    hp, names = [], []                                   # the last block's conv1x1_out gets no gradient: left out of the lists
    hip_names = {id(m): k for k, m in hip.named_modules()}
    for h, r in pairs(hip, ref):
        if h is not hip.conv_layers[LAYERS - 1].conv1x1_out:
            hp += [h.weight_g, h.weight_v] + ([h.bias] if h.bias is not None else [])
            names += [hip_names[id(h)] + '.' + n for n in ['weight_g', 'weight_v'] + (['bias'] if h.bias is not None else [])]

    rp = ref_params(ref)
    assert len(rp) == len(hp) == len(names)

    def hip_step():
        losses, _ = pwg_generator_losses(hip, disc, stft, x, c, y, lambda_adv=4.0, adversarial=True)
        return torch.autograd.grad(losses['total'], hp)

    def ref_step():
        y_ = ref(x, c)
        sc, mag = stft(y_.squeeze(1), y.squeeze(1))
        return torch.autograd.grad(sc + mag + 4.0 * generator_loss([disc(y_)]), rp)

    if args.profile_loop:
        for _ in range(args.profile_loop):
            hip_step()
        torch.cuda.synchronize()
        return
    n0 = PT.launch_count()
    gh = hip_step()
    launches = PT.launch_count() - n0
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    gr = ref_step()
    with torch.no_grad():
        dy = float((hip(x, c) - ref(x, c)).abs().max())
    agree, bad = compare_gradients(names, gh, gr, hip.first_conv)
    losses, y_ = pwg_generator_losses(hip, disc, stft, x, c, y, lambda_adv=4.0, adversarial=True)
    g_up, = torch.autograd.grad(losses['total'], y_)
    acc64, acc_hip, acc_ref = against_float64(names, hip, ref, hp, rp, x, c, g_up.detach())
    del losses, y_, g_up
    torch.cuda.empty_cache()
    if not (acc_hip <= ACCURATE and acc_ref <= ACCURATE):
        print('\n'.join(acc64))
        raise SystemExit(f'pwg_gen_timing: a variant is further than {ACCURATE:g} from float64 on its own ReLU masks: no ratio is reported')
    if bad:
        print('\n'.join(agree + acc64))
        raise SystemExit(f'pwg_gen_timing: the two variants do not compute the same gradients ({", ".join(bad)}): no ratio is reported')
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
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(args.windows):
        for name, fn in variants:                                # alternating
            times[name].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in times.items()}
    flop_fwd = 2.0 * 128 * (192 + AUX + 64) * LAYERS * B * T
    flop = 3.0 * flop_fwd
    saved = 4.0 * (64 + 128) * LAYERS * B * T
    mfma_ms, hbm_ms = flop / 157e12 * 1e3, 2.0 * saved / 6.3e12 * 1e3
    lines = [f'ParallelWaveGAN generator step (forward_train + STFT loss + adversarial term + backward to every generator parameter), B x T = {B} x {T}',
             f'device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library build {binary_id()[:16]}',
             f'{args.windows} alternating windows of >= {args.min_seconds} s device time per variant, device events; median (min .. max) ms per step',
             f'library launches of the generator per hip step: {launches} (the objective\'s operators and the torch glue - weight norm and its '
             f'gradient, stacking the matrices - not counted); peak device memory of one eager hip step {peak:.2f} GiB',
             f'max |y_hip - y_torch| = {dy:.2e}; the two variants\' gradients, per tensor (max |grad_hip - grad_torch| / max |grad_torch|; '
             f'the eight largest):'] + agree
    lines += ['each variant against a float64 copy of the torch generator on the device, the same dL/dy sent back through all (per tensor max '
              f'|grad - grad64| / max |grad64|; limit {ACCURATE:g} on the variant\'s own masks):'] + acc64
    for name, _ in variants:
        v = times[name]
        lines.append(f'  {name:12s} {med[name]:8.3f}  ({min(v):.3f} .. {max(v):.3f})')
    lines.append(f'hip eager / torch eager = {med["hip eager"] / med["torch eager"]:.3f}   hip graph / torch eager = {med["hip graph"] / med["torch eager"]:.3f}')
    lines.append(f'shape-derived bounds of the generator alone: {flop / 1e12:.2f} TFLOP on the fp32 MFMA = {mfma_ms:.2f} ms at 157 TF; saved state '
                 f'{saved / 1e9:.2f} GB written once and read once = {hbm_ms:.2f} ms at 6.3 TB/s')
    for name in ('hip eager', 'hip graph'):
        lines.append(f'{name}: the MFMA bound is {100 * mfma_ms / med[name]:.1f} % of the step, the saved-state traffic bound {100 * hbm_ms / med[name]:.1f} %')
    if med['hip graph'] > med['torch eager']:
        lines.append('THE HIP PATH IS SLOWER THAN TORCH EAGER at this shape (see the kernel trace for the kernel that costs it)')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
