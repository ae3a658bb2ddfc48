"""Developer tool (GPU): the HiFi-GAN multi-scale discriminator at the reference's training shape (configs/tts/hifigan.yaml: max_sentences 16,
max_samples 8192), timed with device events, EAGER calls only (recording these operators into a captured graph is unverified, unsupported and not
done here):

    forward             MultiScaleDiscriminator(y, y_hat): three scale discriminators over both inputs, train() mode
    forward+backward    one discriminator step: discriminator_loss of the outputs, gradients of every parameter
    grouped layers      the five grouped layers of one DiscriminatorS on their own through the C ABI at 2 B = 32 rows: forward, data gradient,
                        weight gradient, with the achieved TFLOP/s and the fraction of the 155 TFLOP/s fp32-MFMA peak

beside the torch twin of tests/hifigan_disc_helpers.py on the same GPU (PyTorch-ROCm eager: Conv1d under torch's spectral / weight norm) - the only
baseline there is.  Every variant is warmed; the figure is the median over alternating windows.

    python tools/hifigan_msd_timing.py [--out profiles/hifigan_msd_timing.txt] [--windows 3] [--batch 16] [--samples 8192]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.hifigan_mpd_timing import PEAK_TF, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hifigan_msd_timing.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--samples', type=int, default=8192)
    ap.add_argument('--min-seconds', type=float, default=0.25)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hifigan_msd_timing: needs the GPU (a timing taken anywhere else says nothing)')
    import warnings
    warnings.filterwarnings('ignore', category=FutureWarning)
    import torch.nn.functional as F
    from diffsinger_amd import MultiScaleDiscriminator, _lib, discriminator_loss
    from diffsinger_amd import hifigan_disc as HD
    from diffsinger_amd.build import binary_id
    from tests import hifigan_disc_helpers as DH
    dev, B, T = 'cuda', args.batch, args.samples
    lib = _lib.load()
    state = DH.synth_state(DH.module_shapes(), 1)
    hip, twin = MultiScaleDiscriminator(), DH.TwinMSD()
    hip.load_state_dict(state, strict=True)
    twin.load_state_dict(state, strict=True)
    hip, twin = hip.to(dev).train(), twin.to(dev).train()
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
        loss = sum(torch.mean((1 - r) ** 2) for r in rs) / 3 + sum(torch.mean(g ** 2) for g in gs) / 3
        return torch.autograd.grad(loss, tp)

    n0 = HD.launch_count()
    hip_fwd()
    launches_f = HD.launch_count() - n0
    hip.load_state_dict(state, strict=True)                     # the forward moved the spectral buffers: both modules start from the same state
    n0 = HD.launch_count()
    gh = hip_step()
    launches = HD.launch_count() - n0
    gt = twin_step()
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gh, gt))
    del gh, gt
    fwd_flop = sum(2.0 * co * (ci // g) * k * 2 * B * DH.lengths(t)[l] for t in (T, T // 2, T // 4) for l, (ci, co, k, _, g) in enumerate(DH.LAYERS))
    res = measure([('hip forward', hip_fwd), ('torch forward', twin_fwd), ('hip forward+backward', hip_step), ('torch forward+backward', twin_step)],
                  args.windows, args.min_seconds)
    lines = [f'HiFi-GAN multi-scale discriminator, B x T = {B} x {T}, y and y_hat ({2 * B} rows per scale), train() mode, eager, device events',
             f'device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, library build {binary_id()[:16]}',
             f'{args.windows} alternating windows of >= {args.min_seconds} s device time per variant; median (min .. max) ms',
             f'library launches: forward {launches_f}, discriminator step {launches}; worst parameter gradient, max |hip - torch| / max |torch| = {worst:.2e}',
             f'counted work: forward {fwd_flop / 1e9:.1f} GFLOP, discriminator step {3 * fwd_flop / 1e12:.3f} TFLOP = {3 * fwd_flop / PEAK_TF / 1e9:.2f} ms at {PEAK_TF:.0f} TFLOP/s']
    for name, flop in (('hip forward', fwd_flop), ('torch forward', fwd_flop), ('hip forward+backward', 3 * fwd_flop), ('torch forward+backward', 3 * fwd_flop)):
        m, lo, hi = res[name]
        lines.append(f'  {name:24s} {m:9.3f}  ({lo:.3f} .. {hi:.3f})   {flop / m / 1e9:7.2f} TFLOP/s = {100 * flop / m / 1e9 / PEAK_TF:5.1f} % of the peak')
    for a, b in (('hip forward', 'torch forward'), ('hip forward+backward', 'torch forward+backward')):
        r = res[a][0] / res[b][0]
        lines.append(f'{a} / {b} = {r:.3f}' + ('   THE HIP PATH IS SLOWER THAN TORCH EAGER HERE' if r > 1 else ''))

    # ---- the grouped layers of one discriminator at full rate, on their own ----
    lines.append('grouped layers at 2 B rows, scale 0: ms (TFLOP/s, % of the peak) hip | torch; fwd = dsv_hgs_gconv / F.conv1d + leaky_relu, dgrad =')
    lines.append('dsv_hgs_gconv_dgrad / conv_transpose1d, wgrad = dsv_hgs_gconv_wgrad (with the bias gradient) / conv1d_weight; packing is not in these figures')
    s = torch.cuda.current_stream().cuda_stream
    ls = DH.lengths(T)
    R = 2 * B
    for l in range(1, 6):
        ci, co, k, S, g = DH.LAYERS[l]
        Li, Lo = ls[l - 1], ls[l]
        x = torch.randn(R, ci, Li, device=dev)
        w = torch.randn(co, ci // g, k, device=dev) / (ci // g * k) ** 0.5
        bias = torch.zeros(co, device=dev)
        out = torch.empty(R, co, Lo, device=dev)
        gr = torch.randn(R, co, Lo, device=dev)
        dxb, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(co, device=dev)
        pf = torch.empty(lib.dsv_hgs_packed_floats(ci, co, S, g, 0), device=dev)
        pb = torch.empty(lib.dsv_hgs_packed_floats(ci, co, S, g, 1), device=dev)
        _lib.check(lib.dsv_hgs_pack(w.data_ptr(), pf.data_ptr(), ci, co, S, g, 0, s))
        _lib.check(lib.dsv_hgs_pack(w.data_ptr(), pb.data_ptr(), ci, co, S, g, 1, s))
        nws = lib.dsv_hgs_wgrad_workspace_floats(R, ci, co, Lo, S, g)
        wsw = torch.empty(max(nws, 1), device=dev)
        variants = [
            ('hip fwd', lambda: _lib.check(lib.dsv_hgs_gconv(x.data_ptr(), pf.data_ptr(), bias.data_ptr(), out.data_ptr(), R, ci, co, Li, S, g, 0.1, s))),
            ('torch fwd', lambda: F.leaky_relu(F.conv1d(x, w, bias, stride=S, padding=20, groups=g), 0.1)),
            ('hip dgrad', lambda: _lib.check(lib.dsv_hgs_gconv_dgrad(gr.data_ptr(), pb.data_ptr(), None, x.data_ptr(), dxb.data_ptr(), R, ci, co, Li, S, g, 0.1, s))),
            ('torch dgrad', lambda: F.conv_transpose1d(gr, w, None, stride=S, padding=20, output_padding=Li - ((Lo - 1) * S + 1), groups=g)),
            ('hip wgrad', lambda: _lib.check(lib.dsv_hgs_gconv_wgrad(gr.data_ptr(), x.data_ptr(), wsw.data_ptr() if nws else None, dw.data_ptr(), db.data_ptr(),
                                                                     R, ci, co, Li, S, g, s))),
            ('torch wgrad', lambda: torch.nn.grad.conv1d_weight(x, w.shape, gr, stride=S, padding=20, groups=g)),
        ]
        r = measure(variants, args.windows, args.min_seconds / 5)
        flop = 2.0 * co * (ci // g) * k * R * Lo
        cells = []
        for op in ('fwd', 'dgrad', 'wgrad'):
            a, b = r[f'hip {op}'][0], r[f'torch {op}'][0]
            cells.append(f'{op} {a:6.3f} ({flop / a / 1e9:5.1f} TF, {100 * flop / a / 1e9 / PEAK_TF:4.1f} %) | {b:6.3f} ({flop / b / 1e9:5.1f} TF)')
        lines.append(f'  l={l} {ci:4d}->{co} S={S} g={g:2d} L {Li:4d}->{Lo:4d} {flop / 1e9:5.1f} GFLOP: ' + '   '.join(cells))
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
