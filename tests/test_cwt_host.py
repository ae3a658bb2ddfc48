"""CPU: the yardsticks of tests/test_gpu_cwt.py are what they claim to be.

  * the float64 restatements of tests/cwt_helpers.py equal the reference's own cwt2f0_norm / add_pitch_loss (run live, in a child process, where
    the reference tree is mounted) and the committed fixture tests/golden/cwt_pitch.npz, which holds the results of the same run;
  * the restated live-frames variant is the frame_keep expression of diffsinger_amd/fs2.py in float64, and a forward over a longer allocation
    with the same live frames equals the shorter one on the frames they share;
  * the case tables hold the shapes they are there for: B 1 and 3, T 2 / 3 / 33 / 63 / 64 / 65 and kCwtBlock - 1 / + 0 / + 1 / twice + 1 (the
    block size is parsed from csrc/fs2_cwt.hpp), T_out - T 0 / 1 / 7, live T / T - 1 / 2, both layouts, both normalisations, both std scales;
    the loss table l1 / l2, with and without uv, both layouts, the three masks, and the sizes at which the loss kernels' grids wrap;
  * no table case has fewer than two live frames (the reference divides by a zero deviation there), and every reference value is finite."""
import os

import numpy as np
import pytest
import torch

from oracle.ref_driver import reference_available
from tests import cwt_helpers as H

F64 = torch.float64
FWD, LOSS = H.fwd_cases(), H.loss_cases()


def _fwd64(c, o, live=None):
    return H.cwt2f0_norm_ref(o['parent'][:, :, :10].double(), o['mean'].double(), o['std'].double(), c.T + c.pad, H.HP_NORM[c.norm], c.std_scale, live)


def _check_against(g):
    for i in range(len(H.GOLDEN_FWD)):
        c, o, want = H.golden_fwd(g, i)
        got = _fwd64(c, o)
        assert got.shape == want.shape == (c.B, c.T + c.pad) and bool(torch.isfinite(want).all())
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (i, c)
    for i in range(len(H.GOLDEN_LOSS)):
        c, hp, o, keys, vals = H.golden_loss(g, i)
        L = H.restate_loss(o, hp)
        assert list(L) == keys, (list(L), keys)
        for k, v in zip(keys, vals):
            assert np.isfinite(float(v)) and abs(float(L[k]) - float(v)) <= 1e-12 * max(abs(float(v)), 1.0), (i, k, float(L[k]), float(v))


@pytest.mark.skipif(not reference_available(), reason='the reference tree is not mounted')
def test_restatement_equals_the_live_reference(tmp_path):
    g = H.run_reference(os.path.join(tmp_path, 'live.npz'))
    _check_against(g)
    committed = H.load_golden()
    assert set(g) == set(committed)
    for k in g:                                                  # the committed fixture is what the reference gives today
        assert g[k].dtype == committed[k].dtype and np.array_equal(g[k], committed[k]), k


def test_restatement_equals_the_committed_fixture():
    g = H.load_golden()
    assert os.path.getsize(H.GOLDEN) < 256 * 1024
    _check_against(g)
    assert {tuple(H.GOLDEN_LOSS[i][1].items()) != () for i in range(len(H.GOLDEN_LOSS))} == {True, False}      # with and without the f0 term
    assert 'f0' in [str(k) for k in g['loss2_keys']] and 'uv' in [str(k) for k in g['loss0_keys']]
    for i, c in enumerate(H.GOLDEN_FWD):
        assert c.B <= 3 and c.T <= 70 and c.live == c.T
    for c, _ in H.GOLDEN_LOSS:
        assert c.B <= 3 and c.T <= 70


def test_forward_table_holds_the_shapes():
    blk = H.BLOCK
    assert blk == 256 and blk % 64 == 0
    src = open(H.HEADER).read()
    assert src.count('__launch_bounds__(kCwtBlock)') == 5 and 'dim3(kCwtBlock)' in src
    assert len(set(FWD)) == len(FWD)
    assert {c.B for c in FWD} == {1, 3}
    want_T = {2, 3, 33, 63, 64, 65, blk - 1, blk, blk + 1, 2 * blk + 1}
    for B in (1, 3):
        assert {c.T for c in FWD if c.B == B} == want_T
        for T in want_T:
            here = [c for c in FWD if c.B == B and c.T == T]
            assert {c.pad for c in here} == {0, 1, 7}
            assert {c.live for c in here} == {v for v in (T, T - 1, 2) if v >= 2}
            assert {(c.pad, c.live) for c in here} == {(p, v) for p in (0, 1, 7) for v in (T, T - 1, 2) if v >= 2}
            assert {c.layout for c in here} == set(H.LAYOUTS) and {c.norm for c in here} == {'log', 'standard'}
            assert len(here) < 4 or {c.std_scale for c in here} == {1.0, 0.8}
    cross = {(c.layout, c.norm, c.std_scale, c.live) for c in FWD if (c.B, c.T, c.pad) == (3, 65, 7)}
    assert cross >= {(lay, n, s, v) for lay in H.LAYOUTS for n in ('log', 'standard') for s in (1.0, 0.8) for v in (65, 64, 2)}
    assert all(c.live >= 2 for c in FWD)                           # live = 1: the reference divides 0 by 0


def test_forward_operands_and_references():
    for c in FWD:
        o = H.fwd_operands(c)
        assert o['parent'].shape == (c.B, c.T, 11 if c.layout == 'view11' else 10) and o['mel2ph'].shape == (c.B, c.T + c.pad)
        owned = (o['mel2ph'] > 0).any(0)
        assert int(owned.nonzero().max()) + 1 == c.live and bool(owned[:c.live].all())          # the last columns are owned by no row
        assert 0.1 <= float(o['std'].min()) and float(o['std'].max()) <= 0.6
        if c.B == 3:
            assert float(o['mean'].max() - o['mean'].min()) == 1.5                                # 6.0 beside 7.5
        ref = _fwd64(c, o, c.live)
        assert bool(torch.isfinite(ref).all())
        assert torch.equal(ref[:, c.T:], ref[:, c.T - 1:c.T].expand(-1, c.pad))
    assert {float(H.fwd_operands(c)['mean'][0]) for c in FWD if c.B == 1} == {6.0, 7.5}


def test_live_variant_is_the_frame_keep_expression():
    """cwt2f0_norm_ref(live=n) against the masked form of diffsinger_amd/fs2.py in float64, and against the forward of the first n frames alone."""
    for c in [c for c in FWD if c.B == 3 and c.T in (3, 65, 257)]:
        o = H.fwd_operands(c)
        s, m, sd = o['parent'][:, :, :10].double(), o['mean'].double(), o['std'].double() * c.std_scale
        keep = (torch.arange(c.T) < c.live).double()[None].expand(c.B, c.T)
        today = H.cwt2f0_norm_today(s, m, sd, c.T + c.pad, H.HP_NORM[c.norm], fk=(keep, torch.tensor(float(c.live), dtype=F64)))
        ref = _fwd64(c, o, c.live)
        assert float((today - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), c
        short = H.cwt2f0_norm_ref(s[:, :c.live], m, sd, c.live, H.HP_NORM[c.norm])
        assert float((short - ref[:, :c.live]).abs().max()) <= 1e-12 * float(ref.abs().max()), c


def test_loss_table_holds_the_shapes():
    assert len(set(LOSS)) == len(LOSS)
    small = {(c.loss, c.use_uv, c.layout, c.mask) for c in LOSS if (c.B, c.T) == (3, 33)}
    assert small == {(lo, u, lay, m) for lo in ('l1', 'l2') for u in (True, False) for lay in H.LAYOUTS for m in ('ragged', 'one_live', 'row_padded')}
    n = {c.B * c.T for c in LOSS}
    assert {H.BLOCK - 1, H.BLOCK, H.BLOCK + 1} <= n and 2 in n
    assert any(H.LOSS_BLOCKS * H.BLOCK < v <= H.LOSS_BWD_BLOCKS * H.BLOCK for v in n) and any(v > H.LOSS_BWD_BLOCKS * H.BLOCK for v in n)
    assert f'std::min<long long>({H.LOSS_BWD_BLOCKS},' in open(H.HEADER).read()
    for c in LOSS:
        if c.B * c.T > 70000:
            continue                                                # the operands of the two large cases are checked where they run
        o = H.loss_operands(c)
        rows = (o['mel2ph'] != 0).sum(1)
        assert o['cwt'].shape == (c.B, c.T, 11 if c.use_uv else 10) and int(rows.sum()) > 0
        assert (c.layout == 'contig') == o['cwt'].is_contiguous()
        if c.mask == 'one_live':
            assert int(rows[-1]) == 1
        if c.mask == 'row_padded':
            assert int(rows[-1]) == 0
        if c.use_uv:
            logit = o['cwt'][:, :, 10]
            assert float(logit.max()) == 30.0 and float(logit.min()) == -30.0
            assert float(o['uv'][0, 0]) == 0.0 and float(o['uv'][0, 1]) == 1.0 and int(o['mel2ph'][0, 0]) != 0 and int(o['mel2ph'][0, 1]) != 0
        L = H.restate_loss(o, H.loss_hp(c))
        assert list(L) == (['C', 'uv', 'f0_mean', 'f0_std'] if c.use_uv else ['C', 'f0_mean', 'f0_std'])
        assert all(np.isfinite(float(v)) for v in L.values())
        if c.use_uv:
            assert float(L['uv']) > 30.0 * 1.3 / float(rows.sum())         # a BCE of 30 is in the sum: exp(30) would have overflowed nothing, exp(-30) underflows nothing
