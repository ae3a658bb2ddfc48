"""GPU: the persistent K-step loop with the dilated convolution as Winograd F(2,3) along the frame axis (csrc/dsd_loop_wino.hpp; the default of
the persistent path) against the reference-generated fixtures, the oracle and the direct-form loop (k_loop, the bit-identity anchor of the
per-layer kernels).  Same dtype as the reference (fp32 in, exact-fp32 MFMA, fp32 transforms); what differs from the direct form is the
reduction order and one rounding per transformed operand - bounded here at 3e-5 on K = 100 loops, a third of the 1e-4 parity budget, which
itself is asserted against the reference's own outputs."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _infer(gd, case, inp, cond, k_step):
    with torch.no_grad():
        if case['kind'] == 'plms':
            return gd.inference(cond, x_T=inp['x_T'].cuda(), K_step=k_step, pndm_speedup=case['interval'])
        if case['gaussian']:
            return gd.inference(cond, x_T=inp['x_T'].cuda(), noise=inp['noise'].cuda(), K_step=k_step, pndm_speedup=0)
        return gd.inference(cond, fs2_mels=inp['fs2_mel'].cuda(), q_noise=inp['q_noise'].cuda(), noise=inp['noise'].cuda(), K_step=k_step,
                            pndm_speedup=0, gaussian_start=False)


@pytest.mark.parametrize('name', ['ddpm_lj_k100', 'shallow_opencpop_k60', 'shallow_popcs_k51', 'plms_opencpop_i40', 'plms_opencpop_i250'])
def test_winograd_loop_vs_reference_fixtures_and_the_direct_loop(name):
    from tests.gpu_helpers import build_hip
    case, pre, cfg, k_step, inp, smin, smax = H.case_setup(name)
    gd, _, _ = build_hip(case['preset'], k_step)
    cond = inp['cond'].transpose(1, 2).contiguous().cuda().transpose(1, 2)
    eng = gd._engine(cond)
    eng.set_loop_mode(1)
    assert eng.loop_mode() == 1 and eng.conv_mode() == 1, 'Winograd is the default convolution of the persistent loop'
    out = _infer(gd, case, inp, cond, k_step).cpu().numpy()
    assert eng.loop_timeouts() == 0
    eng.set_conv_mode('direct')
    assert eng.conv_mode() == 0
    direct = _infer(gd, case, inp, cond, k_step).cpu().numpy()
    eng.set_conv_mode('winograd')
    again = _infer(gd, case, inp, cond, k_step).cpu().numpy()            # cp is re-laid for the other form and back: same bits
    np.testing.assert_array_equal(out, again)
    g = H.load_golden(name)['out']
    scale = max(1.0, float(np.abs(g).max())) if 'plms' in name else 1.0
    e_g, e_d, e_gd = float(np.abs(out - g).max()) / scale, float(np.abs(out - direct).max()) / scale, float(np.abs(direct - g).max()) / scale
    print(f'{name}: Winograd loop vs reference fixture {e_g:.3e} (direct loop {e_gd:.3e}), Winograd vs direct {e_d:.3e}')
    assert e_g <= 1e-4 and e_d <= 3e-5
    assert e_g <= 4.0 * max(e_gd, 2e-6), 'the Winograd form should not be more than a few times the direct form\'s distance from the reference'


@pytest.mark.parametrize('B,T,K', [(8, 1024, 12), (5, 2048, 6), (3, 1000, 8), (2, 33, 5), (1, 5, 3)])
def test_winograd_loop_full_width_all_dilations(B, T, K):
    """Bench-size batches (256 workgroups at once), chunks of whole utterances, ragged T, a two-tile utterance with a one-frame tail, a one-tile
    utterance - dilation cycle 4 (d = 1, 2, 4, 8: every pair order, halos up to 8 frames) against the direct loop."""
    import diffsinger_amd
    from diffsinger_amd import hparams
    from diffsinger_amd.synth import presets
    pre = presets()['opencpop_ds60_rel']
    hparams.clear()
    diffsinger_amd.use_preset('opencpop_ds60_rel')
    torch.manual_seed(3)
    net = diffsinger_amd.DIFF_DECODERS['wavenet'](hparams)
    torch.nn.init.normal_(net.output_projection.weight, std=0.02)
    gd = diffsinger_amd.GaussianDiffusion(None, 80, net, timesteps=100, K_step=K, loss_type='l1', spec_min=pre['spec_min'],
                                          spec_max=pre['spec_max']).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(5)
    cond = torch.randn(B, T, 256, device='cuda', generator=g).transpose(1, 2)
    x_T = torch.randn(B, 1, 80, T, device='cuda', generator=g)
    noise = torch.randn(K, B, 1, 80, T, device='cuda', generator=g)
    eng = gd._engine(cond)
    eng.set_loop_mode(1)
    outs = {}
    for mode in ('winograd', 'direct'):
        eng.set_conv_mode(mode)
        with torch.no_grad():
            outs[mode] = gd.inference(cond, x_T=x_T, noise=noise, K_step=K, pndm_speedup=0).cpu().numpy()
        assert eng.loop_mode() == 1 and eng.conv_mode() == (1 if mode == 'winograd' else 0)
        assert eng.loop_timeouts() == 0
    assert np.isfinite(outs['winograd']).all()
    d = float(np.abs(outs['winograd'] - outs['direct']).max())
    print(f'{B} x {T}, K = {K}: Winograd vs direct loop max-abs mel difference {d:.3e}')
    assert d <= 1e-5


@pytest.mark.parametrize('preset', ['opencpop_ds60_rel', 'lj_ds_beta6'])
def test_conditioner_projection_grouped_by_dilation_gives_the_same_bits(preset):
    """Round 6: for batches that fill the chip a k_condproj workgroup stages (and, Winograd order, re-lays) its conditioner tile once for all
    the layers of one dilation instead of once per layer (grid.y = a multiple of the dilation cycle's period; DSD_CP_GROUPS=layer keeps one
    layer per workgroup).  The same contraction per (layer, tile): both accumulator orders, both presets (cycle 4 / cycle 1) - the same bits."""
    import os
    import diffsinger_amd
    from diffsinger_amd import hparams
    from diffsinger_amd.synth import presets
    pre = presets()[preset]
    hparams.clear()
    diffsinger_amd.use_preset(preset)
    torch.manual_seed(13)
    net = diffsinger_amd.DIFF_DECODERS['wavenet'](hparams)
    torch.nn.init.normal_(net.output_projection.weight, std=0.02)
    B, T, K = 8, 1024, 3
    gd = diffsinger_amd.GaussianDiffusion(None, 80, net, timesteps=100, K_step=K, loss_type='l1', spec_min=pre['spec_min'],
                                          spec_max=pre['spec_max']).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(15)
    cond = torch.randn(B, T, 256, device='cuda', generator=g).transpose(1, 2)
    x_T = torch.randn(B, 1, 80, T, device='cuda', generator=g)
    noise = torch.randn(K, B, 1, 80, T, device='cuda', generator=g)
    eng = gd._engine(cond)
    eng.set_loop_mode(1)
    outs = {}
    try:
        for groups in ('layer', None):
            if groups:
                os.environ['DSD_CP_GROUPS'] = groups
            else:
                os.environ.pop('DSD_CP_GROUPS', None)
            for mode in ('direct', 'winograd'):                     # every switch of the convolution re-lays cp: a fresh k_condproj launch
                eng.set_conv_mode(mode)
                with torch.no_grad():
                    outs[groups, mode] = gd.inference(cond, x_T=x_T, noise=noise, K_step=K, pndm_speedup=0).cpu().numpy()
                assert eng.loop_timeouts() == 0
    finally:
        os.environ.pop('DSD_CP_GROUPS', None)
    for mode in ('direct', 'winograd'):
        assert np.isfinite(outs[None, mode]).all()
        np.testing.assert_array_equal(outs[None, mode], outs['layer', mode], err_msg=mode)


def test_results_do_not_depend_on_the_touch_lead_and_seeded_noise_matches_explicit_noise():
    """The L2 touch computes nothing: every lead (and off) gives the same bits; the
    in-kernel Philox draw equals the explicit-noise loop fed with the same draws; replays are deterministic."""
    import diffsinger_amd
    from diffsinger_amd import hparams
    from diffsinger_amd.synth import presets
    pre = presets()['opencpop_ds60_rel']
    hparams.clear()
    diffsinger_amd.use_preset('opencpop_ds60_rel')
    torch.manual_seed(7)
    net = diffsinger_amd.DIFF_DECODERS['wavenet'](hparams)
    torch.nn.init.normal_(net.output_projection.weight, std=0.02)
    B, T, K, seed = 8, 1000, 6, 24681357
    gd = diffsinger_amd.GaussianDiffusion(None, 80, net, timesteps=100, K_step=K, loss_type='l1', spec_min=pre['spec_min'],
                                          spec_max=pre['spec_max']).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(9)
    cond = torch.randn(B, T, 256, device='cuda', generator=g).transpose(1, 2)
    x_T = torch.randn(B, 1, 80, T, device='cuda', generator=g)
    eng = gd._engine(cond)
    eng.set_loop_mode(1)
    noise = torch.stack([eng.philox_normal(seed, j, B * 80 * T).reshape(B, 1, 80, T) for j in range(K)])
    ref = None
    for touch in (16, 0, 4, 32, 64):
        eng.set_conv_mode('winograd', touch)
        with torch.no_grad():
            out = gd.inference(cond, x_T=x_T, noise=noise, K_step=K, pndm_speedup=0).cpu().numpy()
        assert eng.conv_mode() == 1 and eng.loop_timeouts() == 0
        if ref is None:
            ref = out
        np.testing.assert_array_equal(out, ref, err_msg=f'touch {touch}')
    eng.set_conv_mode('winograd', 16)
    with torch.no_grad():
        seeded = gd.inference(cond, x_T=x_T, K_step=K, pndm_speedup=0, noise_seed=seed).cpu().numpy()
    np.testing.assert_array_equal(seeded, ref)
    assert np.isfinite(ref).all()


# (BASELINE configs[1] at full size - 8 x 1024, K = 100, rows against the oracle - runs on this loop in tests/test_gpu_fullsize.py::
# test_config2_ddpm_k100_rows_vs_oracle_and_row_independence: the default path of that batch IS k_loop_wino_sa; 5.0e-6 / 6.0e-6 in profiles/r5_01_pytest_wino.txt)


def test_starved_winograd_loop_is_loud_and_the_retry_succeeds():
    """The failure protocol of k_loop holds for the Winograd loop: 64 CUs held by a foreign kernel -> spin bound -> RuntimeError at the call
    (check=True), handle parked on the hipGraph path (direct-form per-layer kernels), retry finite and within the forms' distance."""
    import diffsinger_amd
    from diffsinger_amd import hparams
    from diffsinger_amd.synth import presets
    pre = presets()['lj_ds_beta6']
    hparams.clear()
    diffsinger_amd.use_preset('lj_ds_beta6')
    torch.manual_seed(5)
    net = diffsinger_amd.DIFF_DECODERS['wavenet'](hparams)
    torch.nn.init.normal_(net.output_projection.weight, std=0.02)
    B, T, K = 8, 1024, 3
    gd = diffsinger_amd.GaussianDiffusion(None, 80, net, timesteps=100, K_step=K, loss_type='l1', spec_min=pre['spec_min'],
                                          spec_max=pre['spec_max']).cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(8)
    cond = torch.randn(B, T, 256, device='cuda', generator=g).transpose(1, 2)
    x_T = torch.randn(B, 1, 80, T, device='cuda', generator=g)
    noise = torch.randn(K, B, 1, 80, T, device='cuda', generator=g)
    eng = gd._engine(cond)
    eng.set_loop_mode(1)
    run = lambda **kw: gd.inference(cond, x_T=x_T, noise=noise, K_step=K, pndm_speedup=0, **kw)
    ref = run(check=True).cpu().numpy()
    assert eng.loop_mode() == 1 and eng.conv_mode() == 1 and np.isfinite(ref).all()
    side = eng.hold_cus(64, 120000)
    try:
        with pytest.raises(RuntimeError, match='spin bound'):
            run(check=True)
        assert eng.loop_mode() == 0 and eng.conv_mode() == 0       # parked: per-layer kernels
        out = run(check=True).cpu().numpy()                        # the retry, with the holders still resident
        assert np.isfinite(out).all() and float(np.abs(out - ref).max()) <= 1e-5
    finally:
        eng.release_cus()
        side.synchronize()
    eng.set_loop_mode(1)
    np.testing.assert_array_equal(run(check=True).cpu().numpy(), ref)
    assert eng.loop_mode() == 1 and eng.conv_mode() == 1 and eng.loop_timeouts() == 0


def test_default_path_choice_with_the_winograd_loop():
    """Automatic mode, default convolution: small batches keep the latency kernels (G = 16 / 8 / 4 / 2 while every workgroup finds a CU); the
    129-160-tile band that the DIRECT loop left to G = 8 on several grid waves (113-117 ms against its 127) belongs to the Winograd loop
    (104 ms per launch, profiles/r5_03_shape_sweep.jsonl); utterances whose chunking idles 40 % of the chip stay with the per-layer kernels."""
    from tests.gpu_helpers import build_hip
    gd, _, _ = build_hip('lj_ds_beta6', 100)
    want = {(1, 512): (16, 0), (1, 1000): (8, 0), (1, 1550): (4, 0), (4, 777): (2, 0), (3, 1550): (0, 1), (1, 5000): (0, 1), (1, 5200): (0, 1),
            (8, 1024): (0, 1), (5, 1550): (0, 1)}
    for (B, T), (lat, loop) in want.items():
        cond = torch.randn(B, T, 256, device='cuda').transpose(1, 2)
        eng = gd._engine(cond)
        assert (eng.lat_split(), eng.loop_mode()) == (lat, loop), ((B, T), eng.lat_split(), eng.loop_mode())
        assert eng.conv_mode() == (1 if loop or lat in (2, 4, 8) else 0)      # the latency kernels of G = 2 / 4 / 8 run k_lat_conv_w (include/dsd.h)
    cond = torch.randn(3, 5000, 256, device='cuda').transpose(1, 2)       # 157 tiles per utterance: one utterance per persistent launch = 61 % of the chip
    eng = gd._engine(cond)
    assert eng.lat_split() == 0 and eng.loop_mode() == 0 and eng.conv_mode() == 0      # per-layer kernels: 471 tiles = 92 % of two grid waves


# ------------------------------------------------------------------------------------------------------------------------------------------
# the latency kernels with the Winograd convolution (csrc/dsd_lat_wino.hpp: k_lat_conv_w<G>, the default for batches below half the chip)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('preset,layer', [('opencpop_ds60_rel', 0), ('opencpop_ds60_rel', 1), ('opencpop_ds60_rel', 2), ('opencpop_ds60_rel', 3),
                                          ('lj_ds_beta6', 19)])
def test_latency_winograd_layer_against_the_oracle_layer_every_split(preset, layer):
    """ONE residual layer (usr/diff/net.py:66-78) through dsd_debug_layer on k_lat_conv_w<G> + k_lat_out<G> for G = 2 / 4 / 8 (G = 16 keeps the direct
    kernel in either mode), dilations 1 .. 8, ragged T, the last layer (skips only) - against the oracle's layer, next to the direct-form kernels."""
    from oracle import diffnet_oracle as O
    from tests.gpu_helpers import build_hip
    pre = H.presets()[preset]
    cfg = H.net_config(pre)
    gd, _, _ = build_hip(preset, pre['K_step'])
    p = {k: v.detach().cpu() for k, v in gd.denoise_fn.state_dict().items()}
    g = torch.Generator().manual_seed(300 + layer)
    B, T, t = 2, 100, 37
    x = torch.randn(B, 256, T, generator=g)
    cond = torch.randn(B, T, 256, generator=g).transpose(1, 2)
    with torch.no_grad():
        d_emb = O.step_mlp(p, cfg, torch.full((B,), t))
        want_x, want_skip = O.residual_layer(p, cfg, layer, x, cond, d_emb)
    want_skip = want_skip - p[f'residual_layers.{layer}.output_projection.bias'][256:, None]       # the kernels add the skip biases once, in the head
    eng = gd._engine(cond.cuda())
    eng.prepare(cond.cuda())
    eng.set_loop_mode(3)
    last = layer == cfg.residual_layers - 1
    for G in (2, 4, 8, 16):
        eng.set_lat_split(G)
        res = {}
        for conv in ('winograd', 'direct'):
            eng.set_conv_mode(conv)
            assert eng.lat_split() == G
            xo, sk = eng.debug_layer(layer, t, x.cuda())
            res[conv] = float((sk.cpu() - want_skip).abs().max()) if last else max(float((sk.cpu() - want_skip).abs().max()),
                                                                                      float((xo.cpu() - want_x).abs().max()))
        print(f'{preset} layer {layer} (dilation {2 ** (layer % cfg.dilation_cycle_length)}) G={G}: max-abs err vs the oracle layer: Winograd '
              f'{res["winograd"]:.3e}, direct {res["direct"]:.3e}')
        assert res['winograd'] < 2e-5, G
    eng.set_conv_mode('winograd')


def test_one_utterance_k100_on_the_winograd_latency_kernels_vs_oracle_and_timing():
    """The reference's own inference shape - ONE utterance (configs/tts/fs2.yaml:70), here 512 / 1000 / 1550 frames, K = 100 DDPM - on the default
    path (latency kernels; G = 8 / 4 with the Winograd convolution, G = 16 direct in either mode) against the oracle, and its time next to the
    direct-form kernels."""
    import time
    from oracle import diffnet_oracle as O
    from diffsinger_amd.synth import make_inputs
    from tests.gpu_helpers import build_hip
    K = 100
    gd, cfg, pre = build_hip('lj_ds_beta6', K)
    sch = O.make_schedule(H.betas_for(pre))
    smin = torch.tensor(pre['spec_min'], dtype=torch.float32)[None, None, :]
    smax = torch.tensor(pre['spec_max'], dtype=torch.float32)[None, None, :]
    p = H.oracle_params(cfg)
    for T, G in ((512, 16), (1000, 8), (1550, 4)):
        inp = make_inputs(70 + G, 1, T, n_noise=K)
        cond, x_T, noise = inp['cond'].cuda(), inp['x_T'].cuda(), inp['noise'].cuda()
        eng = gd._engine(cond)
        outs, ms = {}, {}
        for conv in ('winograd', 'direct'):
            eng.set_conv_mode(conv)
            assert eng.lat_split() == G and eng.loop_mode() == 0
            with torch.no_grad():
                outs[conv] = gd.inference(cond, x_T=x_T, noise=noise, K_step=K, pndm_speedup=0).clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    gd.inference(cond, x_T=x_T, noise=noise, K_step=K, pndm_speedup=0)
                torch.cuda.synchronize()
            ms[conv] = (time.perf_counter() - t0) / 3 * 1e3
        eng.set_conv_mode('winograd')
        err = None      # (against the oracle: tests/test_gpu_fullsize.py runs one utterance of 1024 frames on these kernels, G = 8, from the session's shared oracle row)
        d = float((outs['winograd'] - outs['direct']).abs().max())
        print(f'1 x {T}, K = 100 on the latency kernels G = {G}: Winograd {ms["winograd"]:.1f} ms, direct {ms["direct"]:.1f} ms per call; max-abs mel difference '
              f'{d:.3e}' + (f'; Winograd vs oracle {err:.3e}' if err is not None else ''))
        assert d <= 5e-5 and bool(torch.isfinite(outs['winograd']).all())


# ------------------------------------------------------------------------------------------------------------------------------------------
# Parity margin under stress: Winograd's error grows with the activation magnitude (the transformed operands d0 - d2,
# d1 + d2 ... are sums of activations, the transformed weights sums of taps), and every other parity figure of this repo is taken at
# N(0, kaiming) weights and N(0, 1) conditioners (the reference ships no checkpoint).  Here the residual stack's weights AND the conditioner
# are scaled: x 4 puts the gate pre-activations at ~16 x their usual range.  What the first version of this test (r6_04) showed: at x 4 a K-step
# loop is CHAOTIC - the exact-fp32 direct loop ends 2.6 from the oracle on a mel of range ~10, the Winograd loop 3.1, each 2.8 from the other:
# saturated gates amplify any rounding difference (including the reference's own reduction order) by orders of magnitude per step, so a K-step
# comparison there measures the network's conditioning, not an implementation.  The margin is therefore taken where it is defined: ONE
# evaluation through the loop (K = 1: x_T -> the t = 0 step -> mel), and the growth over K is reported beside it for both forms.
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampler', ['ddpm', 'plms'])
def test_parity_margin_with_scaled_weights_and_conditioner(sampler):
    from oracle import diffnet_oracle as O
    from diffsinger_amd.synth import make_inputs
    from tests.gpu_helpers import build_hip
    preset = {'ddpm': 'lj_ds_beta6', 'plms': 'opencpop_ds1000'}[sampler]               # dilation cycle 1 / cycle 4 (d = 1, 2, 4, 8)
    B, T = 4, 256                                                                         # 32 tiles on the persistent loop (forced)
    rows = []
    for scale_w in (1.0, 2.0, 4.0):
        for K in ((1, 4) if sampler == 'ddpm' else (1000,)):       # (K = 16 at x 2 measured 1.8e-2 / 2.1e-2 in r6_06: chaos in both forms)
            gd, cfg, pre = build_hip(preset, K)
            p = {k: v.clone() for k, v in H.oracle_params(cfg).items()}
            scaled = [k for k in p if k.startswith('residual_layers.') and k.endswith('weight')]
            assert len(scaled) == 4 * cfg.residual_layers
            for k in scaled:
                p[k] *= scale_w
            gd.denoise_fn.load_state_dict(p, strict=True)
            inp = make_inputs(900 + K, B, T, n_noise=K if sampler == 'ddpm' else 0)
            inp['cond'] = inp['cond'] * scale_w
            sch = O.make_schedule(H.betas_for(pre))
            smin = torch.tensor(pre['spec_min'], dtype=torch.float32)[None, None, :]
            smax = torch.tensor(pre['spec_max'], dtype=torch.float32)[None, None, :]
            cond = inp['cond'].transpose(1, 2).contiguous().cuda().transpose(1, 2)
            eng = gd._engine(cond)
            eng.set_loop_mode(1)
            intervals = (1000,) if sampler == 'plms' else (0,)                           # PLMS: ONE iteration = two evaluations (x_T -> x_0 in one step)
            for interval in intervals:
                outs = {}
                for conv in ('winograd', 'direct'):
                    eng.set_conv_mode(conv)
                    assert eng.loop_mode() == 1 and eng.conv_mode() == (1 if conv == 'winograd' else 0)
                    with torch.no_grad():
                        if sampler == 'ddpm':
                            outs[conv] = gd.inference(cond, x_T=inp['x_T'].cuda(), noise=inp['noise'].cuda(), K_step=K, pndm_speedup=0).cpu()
                        else:
                            outs[conv] = gd.inference(cond, x_T=inp['x_T'].cuda(), K_step=K, pndm_speedup=interval).cpu()
                    assert eng.loop_timeouts() == 0
                eng.set_conv_mode('winograd')
                with torch.no_grad():
                    if sampler == 'ddpm':
                        want = O.infer_mel(p, cfg, sch, inp['cond'], smin, smax, k_step=K, noises=list(inp['noise']), x_T=inp['x_T'])
                    else:
                        want = torch.cat([O.infer_mel(p, cfg, sch, inp['cond'][b:b + 1], smin, smax, k_step=K, x_T=inp['x_T'][b:b + 1], pndm_interval=interval)
                                          for b in range(B)])                             # (the reference's PLMS is B = 1 only)
                scale = max(1.0, float(want.abs().max())) if sampler == 'plms' else 1.0  # PLMS has no clamp: graded relative to max|mel| (quirk 4)
                e = {k: float((v - want).abs().max()) / scale for k, v in outs.items()}
                rows.append((scale_w, K, e['winograd'], e['direct']))
                evals = K if sampler == 'ddpm' else 2
                print(f'{sampler} ({preset}, {B} x {T}), stack weights and cond x {scale_w:g}, {evals} evaluation(s): max-abs mel err vs the oracle: Winograd loop '
                      f'{e["winograd"]:.3e} (margin {1e-4 / max(e["winograd"], 1e-12):.1f} x under 1e-4), direct loop {e["direct"]:.3e}')
                assert bool(torch.isfinite(outs['winograd']).all())
                # Measured (profiles/r6_06_stress.txt): x 1 - both forms 4.8e-7 (1 evaluation) ... 1.9e-6 (16); x 2 - 1.1e-5 / 6.9e-6 (1), 6.3e-5 / 5.3e-5
                # (4), 1.8e-2 / 2.1e-2 (16); x 4 - ONE evaluation is already 5.8e-2 / 4.7e-2 from the oracle in BOTH forms: with 16 x the
                # activation range the 20-layer stack amplifies a rounding difference ~1e5 x per evaluation - no fp32 implementation (the
                # reference on another BLAS included) is determinate there.  What is asserted: the budget wherever the direct form keeps it,
                # and everywhere that the Winograd form is no further from the oracle than ~2 x the exact-fp32 direct form.
                if e['direct'] <= 5e-5:
                    assert e['winograd'] <= 1e-4
                assert e['winograd'] <= 3.0 * max(e['direct'], 2e-6), (scale_w, evals, e)
                if scale_w == 1.0:
                    assert e['winograd'] <= 1e-5
            del gd
