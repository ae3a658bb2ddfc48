"""Developer tool (GPU): the HiFi-GAN multi-period discriminator at the reference's training shape (configs/tts/hifigan.yaml: max_sentences 16,
max_samples 8192), timed with device events, EAGER calls only (recording these operators into a graph is unverified and not done here):

    forward         MultiPeriodDiscriminator(y, y_hat): the five period discriminators over both inputs
    forward+backward    one discriminator step: discriminator_loss of the outputs, gradients of every parameter
    wide layers     per period the 512 -> 1024 (stride 3) and 1024 -> 1024 (stride 1) layers on their own through the C ABI: forward, data gradient,
                    weight gradient at 2 B = 32 rows, with the achieved TFLOP/s and the fraction of the 155 TFLOP/s fp32-MFMA peak

beside the torch twin of tests/hifigan_mpd_helpers.py on the same GPU (PyTorch-ROCm eager: Conv2d under torch's weight_norm) - the only baseline there
is.  Counts, not measurements: 151 GFLOP forward per input, 0.91 TFLOP for one discriminator step (forward, data and weight gradients over y and
y_hat) = 5.8 ms at the peak.  Every variant is warmed; the figure is the median over alternating windows.

    python tools/hifigan_mpd_timing.py [--out profiles/hifigan_mpd_timing.txt] [--windows 3] [--batch 16] [--samples 8192]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0


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


def measure(variants, windows, min_s):
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(windows):
        for name, fn in variants:
            times[name].append(window(fn, min_s))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hifigan_mpd_timing.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--samples', type=int, default=8192)
    ap.add_argument('--min-seconds', type=float, default=0.25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hifigan_mpd_timing: needs the GPU (a timing taken anywhere else says nothing)')
    import warnings
    warnings.filterwarnings('ignore', category=FutureWarning)
    from diffsinger_amd import MultiPeriodDiscriminator, _lib, discriminator_loss
    from diffsinger_amd import hifigan_disc as HD
    from diffsinger_amd.build import binary_id
    from tests import hifigan_mpd_helpers as MH
    dev, B, T = 'cuda', args.batch, args.samples
    lib = _lib.load()
    state = MH.synth_state(MH.module_shapes(), 1, MH.SLOPE)
    hip, twin = MultiPeriodDiscriminator(), MH.TwinMPD()
    hip.load_state_dict(state, strict=True)
    twin.load_state_dict(state, strict=True)
    hip, twin = hip.to(dev), twin.to(dev)
    gen = torch.Generator().manual_seed(2)
    y = (0.5 * torch.randn(B, 1, T, generator=gen)).to(dev)
    y_hat = (y.cpu() + 0.3 * torch.randn(B, 1, T, generator=gen)).to(dev)
    names = [k for k, _ in hip.named_parameters()]
    hp, tp = [dict(hip.named_parameters())[k] for k in names], [dict(twin.named_parameters())[k] for k in names]

    def hip_fwd():
        with torch.no_grad():
            return hip(y, y_hat)

    def twin_fwd():
        with torch.no_grad():
            return twin(y, y_hat)

    def hip_step():
        rs, gs, _, _ = hip(y, y_hat)
        return torch.autograd.grad(sum(discriminator_loss(rs, gs)), hp)

    def twin_step():
        rs, gs, _, _ = twin(y, y_hat)
        loss = sum(torch.mean((1 - r) ** 2) for r in rs) / 5 + sum(torch.mean(g ** 2) for g in gs) / 5
        return torch.autograd.grad(loss, tp)

    n0 = HD.launch_count()
    gh = hip_step()
    launches = HD.launch_count() - n0
    gt = twin_step()
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gh, gt))
    del gh, gt
    fwd_flop = sum(2.0 * co * ci * k * 2 * B * MH.heights(T, p)[l + 1] * p for p in MH.PERIODS for l, (ci, co, k, _) in enumerate(MH.LAYERS))
    res = measure([('hip forward', hip_fwd), ('torch forward', twin_fwd), ('hip forward+backward', hip_step), ('torch forward+backward', twin_step)],
                  args.windows, args.min_seconds)
    lines = [f'HiFi-GAN multi-period discriminator, B x T = {B} x {T}, y and y_hat (2 B = {2 * B} rows per period), eager, device events',
             f'device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library build {binary_id()[:16]}',
             f'{args.windows} alternating windows of >= {args.min_seconds} s device time per variant; median (min .. max) ms',
             f'library launches per hip discriminator step: {launches}; worst parameter gradient, max |hip - torch| / max |torch| = {worst:.2e}',
             f'counted work: forward {fwd_flop / 1e9:.1f} GFLOP, discriminator step {3 * fwd_flop / 1e12:.3f} TFLOP = {3 * fwd_flop / PEAK_TF / 1e9:.2f} ms at {PEAK_TF:.0f} TFLOP/s']
    for name, flop in (('hip forward', fwd_flop), ('torch forward', fwd_flop), ('hip forward+backward', 3 * fwd_flop), ('torch forward+backward', 3 * fwd_flop)):
        m, lo, hi = res[name]
        lines.append(f'  {name:24s} {m:9.3f}  ({lo:.3f} .. {hi:.3f})   {flop / m / 1e9:7.2f} TFLOP/s = {100 * flop / m / 1e9 / PEAK_TF:5.1f} % of the peak')
    for a, b in (('hip forward', 'torch forward'), ('hip forward+backward', 'torch forward+backward')):
        r = res[a][0] / res[b][0]
        lines.append(f'{a} / {b} = {r:.3f}' + ('   THE HIP PATH IS SLOWER THAN TORCH EAGER HERE' if r > 1 else ''))

    # ---- the two wide layers of every period, on their own ----
    lines.append('wide layers at 2 B rows: ms (TFLOP/s, % of the peak) hip | torch, per period; fwd = dsv_hgp_conv / F.conv2d + leaky_relu, dgrad = dsv_hgp_conv_dgrad /')
    lines.append('conv_transpose2d, wgrad = dsv_hgp_conv_wgrad (with the bias gradient) / conv2d_weight; packing the weights is not in these figures')
    s = torch.cuda.current_stream().cuda_stream
    import torch.nn.functional as F
    for p in MH.PERIODS:
        hs = MH.heights(T, p)
        for l in (3, 4):
            ci, co, k, S = MH.LAYERS[l]
            Hi, Ho, R = hs[l], hs[l + 1], 2 * B
            x = torch.randn(R, ci, Hi, p, device=dev)
            w = torch.randn(co, ci, k, device=dev) / (ci * k) ** 0.5
            bias = torch.zeros(co, device=dev)
            out = torch.empty(R, co, Ho, p, device=dev)
            g = torch.randn(R, co, Ho, p, device=dev)
            dxb, dw, db = torch.empty_like(x), torch.empty(co, ci, k, device=dev), torch.empty(co, device=dev)
            packed = torch.empty(lib.dsv_packed_floats(co, ci, k), device=dev)
            _lib.check(lib.dsv_pack_weight(w.data_ptr(), co, ci, k, packed.data_ptr(), s))
            pd = torch.empty(lib.dsv_hgp_dgrad_packed_offset(ci, co, S, S), device=dev)
            for r in range(S):
                m = lib.dsv_hgp_dgrad_phase_taps(S, r)
                ks = [t for t in range(k) if m >> t & 1]
                mat = w[:, :, ks].permute(1, 0, 2).contiguous()
                _lib.check(lib.dsv_pack_weight(mat.data_ptr(), ci, co, len(ks), pd.data_ptr() + 4 * lib.dsv_hgp_dgrad_packed_offset(ci, co, S, r), s))
            nws = lib.dsv_hgp_wgrad_workspace_floats(R, ci, co, Ho, p)
            wsw = torch.empty(max(nws, 1), device=dev)
            w4 = w[..., None].contiguous()
            variants = [
                ('hip fwd', lambda: _lib.check(lib.dsv_hgp_conv(x.data_ptr(), packed.data_ptr(), bias.data_ptr(), out.data_ptr(), R, ci, co, Hi, p, S, 0.1, s))),
                ('torch fwd', lambda: F.leaky_relu(F.conv2d(x, w4, bias, stride=(S, 1), padding=(2, 0)), 0.1)),
                ('hip dgrad', lambda: _lib.check(lib.dsv_hgp_conv_dgrad(g.data_ptr(), pd.data_ptr(), None, x.data_ptr(), dxb.data_ptr(), R, ci, co, Hi, p, S, 0.1, s))),
                ('torch dgrad', lambda: F.conv_transpose2d(g, w4, None, stride=(S, 1), padding=(2, 0), output_padding=(Hi - ((Ho - 1) * S + 1), 0))),
                ('hip wgrad', lambda: _lib.check(lib.dsv_hgp_conv_wgrad(g.data_ptr(), x.data_ptr(), wsw.data_ptr() if nws else None, dw.data_ptr(), db.data_ptr(), R,
                                                                        ci, co, Hi, p, S, s))),
                ('torch wgrad', lambda: torch.nn.grad.conv2d_weight(x, w4.shape, g, stride=(S, 1), padding=(2, 0))),
            ]
            r = measure(variants, args.windows, args.min_seconds / 5)
            flop = 2.0 * co * ci * k * R * Ho * p
            cells = []
            for op in ('fwd', 'dgrad', 'wgrad'):
                a, b = r[f'hip {op}'][0], r[f'torch {op}'][0]
                cells.append(f'{op} {a:6.3f} ({flop / a / 1e9:5.1f} TF, {100 * flop / a / 1e9 / PEAK_TF:4.1f} %) | {b:6.3f} ({flop / b / 1e9:5.1f} TF)')
            lines.append(f'  p={p:2d} {ci:4d}->{co} S={S} H {Hi:3d}->{Ho:3d} {flop / 1e9:5.1f} GFLOP: ' + '   '.join(cells))
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
