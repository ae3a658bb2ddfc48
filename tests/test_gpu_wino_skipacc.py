"""GPU: the persistent Winograd loop with the running skip sum kept in the out-projection's accumulators (csrc/dsd_loop_wino.hpp: the skip row
blocks are the MFMA's C/D operand across the layers, zeroed at the start of every evaluation, read by the head) and the y-tile staging that
masks only in workgroups whose tile is cut by the end of the utterance.

Shapes: the smallest that reach every path.  Dilation cycle 4 (opencpop_ds60_rel: d = 1, 2, 4, 8) - 2 x 33 frames, 3 evaluations: a full
tile beside a one-frame tail tile (both branches of the staging, of the own frames and of the right halo; the accumulators re-zeroed twice);
1 x 5: one cut tile without neighbours; 2 x 64: full tiles only.  The benchmark's network (lj_ds_beta6, d = 1) at 2 x 96.  One PLMS run
(opencpop_ds1000, 1 x 33, pndm_speedup 250): the other instantiation of the kernel.

Bounds: against the direct-form loop (an unchanged kernel) the 1e-5 of test_gpu_wino.py::test_winograd_loop_full_width_all_dilations at these
K; against the oracle the rule of test_parity_margin_with_scaled_weights_and_conditioner - no further than 3 x the direct form (floor 2e-6),
PLMS relative to max |mel|.  A skip sum that leaks from one evaluation into the next, or a mask left out, is an error of order 1e-1."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = [('opencpop_ds60_rel', 2, 33, 3, 0), ('opencpop_ds60_rel', 1, 5, 2, 0), ('opencpop_ds60_rel', 2, 64, 2, 0), ('lj_ds_beta6', 2, 96, 2, 0),
         ('opencpop_ds1000', 1, 33, 1000, 250)]


@pytest.mark.parametrize('preset,B,T,K,interval', CASES, ids=[f'{c[0]}-{c[1]}x{c[2]}-K{c[3]}' + (f'-plms{c[4]}' if c[4] else '') for c in CASES])
def test_skip_sum_in_the_accumulators_and_cut_tile_staging(preset, B, T, K, interval):
    from oracle import diffnet_oracle as O
    from diffsinger_amd.synth import make_inputs
    from tests.gpu_helpers import build_hip
    plms = interval > 0
    gd, cfg, pre = build_hip(preset, K)
    p = H.oracle_params(cfg)
    inp = make_inputs(1300 + T, B, T, n_noise=0 if plms else K)
    sch = O.make_schedule(H.betas_for(pre))
    smin = torch.tensor(pre['spec_min'], dtype=torch.float32)[None, None, :]
    smax = torch.tensor(pre['spec_max'], dtype=torch.float32)[None, None, :]
    cond = inp['cond'].transpose(1, 2).contiguous().cuda().transpose(1, 2)
    eng = gd._engine(cond)
    eng.set_loop_mode(1)                                                     # the persistent loop, forced (these batches are far below its threshold)

    def run():
        with torch.no_grad():
            if plms:
                return gd.inference(cond, x_T=inp['x_T'].cuda(), K_step=K, pndm_speedup=interval).cpu().numpy()
            return gd.inference(cond, x_T=inp['x_T'].cuda(), noise=inp['noise'].cuda(), K_step=K, pndm_speedup=0).cpu().numpy()

    outs = {}
    for conv in ('winograd', 'direct'):
        eng.set_conv_mode(conv)
        assert eng.loop_mode() == 1 and eng.conv_mode() == (1 if conv == 'winograd' else 0)
        outs[conv] = run()
        assert eng.loop_timeouts() == 0
    eng.set_conv_mode('winograd')
    again = run()
    assert eng.loop_timeouts() == 0
    np.testing.assert_array_equal(outs['winograd'], again)
    with torch.no_grad():
        if plms:
            want = torch.cat([O.infer_mel(p, cfg, sch, inp['cond'][b:b + 1], smin, smax, k_step=K, x_T=inp['x_T'][b:b + 1], pndm_interval=interval)
                              for b in range(B)]).numpy()                    # (the reference's PLMS is B = 1 only)
        else:
            want = O.infer_mel(p, cfg, sch, inp['cond'], smin, smax, k_step=K, noises=list(inp['noise']), x_T=inp['x_T']).numpy()
    # PLMS has no clamp: graded relative to max |mel|, against the direct loop too (as the fixture test of test_gpu_wino.py does) - this mel reaches
    # 184, where one fp32 ulp is 1.5e-5: no two reduction orders agree to an absolute 1e-5 there
    scale = max(1.0, float(np.abs(want).max())) if plms else 1.0
    d = float(np.abs(outs['winograd'] - outs['direct']).max()) / scale
    e = {k: float(np.abs(v - want).max()) / scale for k, v in outs.items()}
    print(f'{preset} {B} x {T}, K = {K}' + (f', PLMS interval {interval}' if plms else '') + f': Winograd vs direct loop {d:.3e} (max |mel| '
          f'{float(np.abs(want).max()):.3g}); vs the oracle: Winograd {e["winograd"]:.3e}, direct {e["direct"]:.3e}')
    assert np.isfinite(outs['winograd']).all()
    assert d <= 1e-5
    assert e['winograd'] <= 3.0 * max(e['direct'], 2e-6), e
