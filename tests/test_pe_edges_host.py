"""CPU: the yardsticks of tests/test_gpu_pe_edges.py are what they claim to be, its cases sit where they are meant to sit, and the bound
catches the bugs it is for.

  * the elementary restatements of tests/pe_edge_helpers.py equal the float64 yardstick (aten, pe_train_helpers.f0_losses) to 1e-12 in float64
    and aten's float32 result to a few ulp on the small shapes of tests/test_gpu_pe_train.py;
  * every case is on the intended side of the kernel constant it is there for, and no ReLU input is near its kink;
  * eight restated bugs exceed the bound (pe_train_helpers.bound of the float32 restatement's own error) 100 x or more on every listed case
    where they can be seen, and are exact where they cannot.  Which of them only the new shapes can see:
      BatchNorm statistics over the first 8192 values of a channel     only where B * TS > 8192: none of the earlier shapes
      f0 loss without the frames from index 65 536 on                  only where B * T > 65 536: none of the earlier shapes
      GroupNorm group sums over the channels c % 4 == 0 only           at every shape with more than one channel per group
      GroupNorm dgamma / dbeta from utterance 0, TS for T, E[x^2] - E[x]^2, the missing (uv == 0) factor     at the earlier shapes too
      biased running_var                                               differs by 1 / n: 100 x the 2e-6 floor needs n < 5000, so the
                                                                       earlier small shapes see it and a training-size batch cannot"""
import pytest
import torch

from tests import pe_edge_helpers as E
from tests import pe_train_helpers as PH

F32, F64 = torch.float32, torch.float64
FEW_ULP = 16 * E.U                               # of the tensor's largest value (pe_train_helpers.rel_err)


def _bn_args(c):
    return (c['x'], c['gamma'], c['beta'], c['rm'], c['rv'], c['keep'], c['dy'], c['relu_in'])


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. the restatements
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', E.BN_SMALL + [(8, 1025)])
@pytest.mark.parametrize('kind', E.BN_KINDS)
def test_batch_norm_restatement(B, T, kind):
    args = _bn_args(E.bn_case(B, T, kind))
    a64, r64 = E.bn_reference(*args, F64), E.bn_restated(*args, F64)
    for k in a64:
        assert PH.rel_err(r64[k], a64[k]) <= 1e-12, (k, PH.rel_err(r64[k], a64[k]))
    # float32 at 3 x 75 only: at length, and with the mean far from zero, aten's double accumulation shows; with two values per channel dx is
    # zero but for rounding, which no two float32 forms share
    if (B, T) == (3, 75) and kind == 'kink_free':
        a32, r32 = E.bn_reference(*args, F32), E.bn_restated(*args, F32)
        for k in a32:
            assert r32[k].dtype == F32
            print(f'bn[{B}x{T}] {k}: restatement against aten, float32: {PH.rel_err(r32[k], a32[k]) / E.U:.1f} u')
            assert PH.rel_err(r32[k], a32[k]) <= FEW_ULP, k


@pytest.mark.parametrize('B,C,G,T', E.GN_SMALL + [(2, 48, 16, 64), (2, 32, 2, 1)])
@pytest.mark.parametrize('plain', [False, True])
def test_group_norm_restatement(B, C, G, T, plain):
    c = E.gn_case(B, C, G, T)
    args = (c['x'], c['gamma'], c['beta'], None if plain else c['res'], c['dy'], G)
    a64, r64 = E.gn_reference(*args, F64, relu=not plain), E.gn_restated(*args, F64, relu=not plain)
    m64 = E.gn_backward_manual(c['x'], c['gamma'], c['beta'], c['dy'], G, F64, relu=not plain)
    assert ('dres' in a64) == (not plain)
    for k in a64:
        assert PH.rel_err(r64[k], a64[k]) <= 1e-12, k
    for k in m64:
        assert PH.rel_err(m64[k], a64[k]) <= 1e-12, k
    if (B, C, G, T) in E.GN_SMALL:
        a32, r32 = E.gn_reference(*args, F32, relu=not plain), E.gn_restated(*args, F32, relu=not plain)
        for k in a32:
            assert r32[k].dtype == F32
            print(f'gn[{B}x{C}/{G}x{T}] {k}: restatement against aten, float32: {PH.rel_err(r32[k], a32[k]) / E.U:.1f} u')
            assert PH.rel_err(r32[k], a32[k]) <= FEW_ULP, k


@pytest.mark.parametrize('pitch_loss,use_uv,Cp', [('l1', True, 2), ('l2', False, 2), ('l1', True, 3)])
def test_f0_loss_restatement(pitch_loss, use_uv, Cp):
    c, hp = E.f0_case(3, 301, Cp), E.f0_hp(pitch_loss, use_uv)
    args = (c['pred'], c['f0'], c['uv'], c['nonpadding'], hp)
    a64, r64 = E.f0_reference(*args, F64), E.f0_restated(*args, F64)
    a32, r32 = E.f0_reference(*args, F32), E.f0_restated(*args, F32)
    assert set(a64) == set(r64) == ({'uv', 'f0', 'dpred'} if use_uv else {'f0', 'dpred'})
    for k in a64:
        assert PH.rel_err(r64[k], a64[k]) <= 1e-12, k
        assert r32[k].dtype == F32 and PH.rel_err(r32[k], a32[k]) <= FEW_ULP, k
    assert float(a64['dpred'][:, :, 2:].abs().sum()) == 0.0


def test_affine_bound_holds_for_both_float32_forms():
    x, a, b, keep = E.affine_case(3, 256, 75, 'ragged')
    want, tol = E.affine_reference(x, a, b, keep)
    plain = (x * a[None, :, None] + b[None, :, None]) * keep[:, None, :]
    fused = torch.addcmul(b[None, :, None].expand_as(x), x, a[None, :, None].expand_as(x)) * keep[:, None, :]
    for got in (plain, fused):
        assert bool(((got.double() - want).abs() <= tol).all())
    assert not bool((((x * a[None, :, None] * 1.000001 + b[None, :, None]) * keep[:, None, :]).double() - want).abs().le(tol).all())


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. the cases are where they are meant to be
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    assert E.kernel_constants() == {'BN_STAGE4': E.BN_STAGE4, 'GN_MAX_CG': E.GN_MAX_CG, 'F0_FWD_FRAMES': E.F0_FWD_FRAMES,
                                    'F0_BWD_FRAMES': E.F0_BWD_FRAMES, 'EW_BLOCKS': E.EW_BLOCKS}
    assert (E.BN_STAGE4, E.GN_MAX_CG, E.F0_FWD_FRAMES, E.F0_BWD_FRAMES, E.EW_BLOCKS) == (2048, 64, 65536, 262144, 16384)


def test_batch_norm_shapes_straddle_the_stage():
    n4 = {(B, T): B * E.fs_ts(T) // 4 for B, T in E.BN_SHAPES}                   # float4s of a channel against kPeBnStage4
    assert n4[8, 1024] == n4[1, 8192] == E.BN_STAGE4 and E.fs_ts(1024) == 1024 and E.fs_ts(8192) == 8192      # the last staged size, no tail
    assert n4[8, 1025] == 8 * 1056 // 4 > E.BN_STAGE4 and n4[1, 8193] == 8224 // 4 > E.BN_STAGE4            # the first unstaged one
    assert [E.bn_staged(B, T) for B, T in E.BN_SHAPES] == [True, False, True, False, False, False]
    assert all(E.bn_staged(B, T) for B, T in E.BN_SMALL + [(3, 47), (2, 40)])    # every earlier test and fixture is staged
    assert 10 * 2000 == 20000 and E.fs_ts(2000) == 2016 and E.fs_ts(8000) == 8000
    for B, T in E.BN_SHAPES:
        for kind in E.BN_KINDS:
            c = E.bn_case(B, T, kind)
            live = c['keep'].sum(1)
            assert c['relu_in'] == (kind == 'kink_free') and float(live.min()) >= 1 and float(c['keep'][:, -1].sum()) == 0
            assert B == 1 or len(set(live.tolist())) == B                        # ragged per row
            if kind == 'kink_free':
                assert float(c['x'].abs().min()) >= 0.01


def test_group_norm_shapes_and_kinks():
    cgs = [C // G for _, C, G, _ in E.GN_SHAPES]
    assert cgs == [16, 16, 16, 1, 3, 64, 16] and max(cgs) == E.GN_MAX_CG       # kPeGnMaxCg; 1 and 3: waves of k_pe_gn_bwd that own nothing
    assert 130 // 2 == E.GN_MAX_CG + 1                                           # the refused shape
    assert [T for _, _, _, T in E.GN_SHAPES if T == E.fs_ts(T)] == [8000, 64, 96]
    for shape in E.GN_SHAPES:
        c = E.gn_case(*shape)
        print(f'gn{shape}: min |v| {c["vmin"]:.2e} after {c["rounds"]} repair rounds')
        assert c['vmin'] >= E.KINK and c['rounds'] <= 20
    c = E.gn_case(1, 16, 1, 8000, offset=True)
    assert c['vmin'] >= E.KINK and abs(float(c['x'].mean()) - 100) < 0.01


def test_pitch_loss_shapes_and_inputs():
    frames = [B * T for B, T in E.F0_SHAPES]
    assert frames[0] <= E.F0_FWD_FRAMES < frames[1] <= E.F0_BWD_FRAMES < frames[2]            # 256 * 256 and 1024 * 256 frames
    assert frames[1] - E.F0_FWD_FRAMES == 4464 and frames[2] - E.F0_BWD_FRAMES == 17856
    for B, T in E.F0_SHAPES:
        c = E.f0_case(B, T)
        np_v = c['nonpadding'] * (c['uv'] == 0)
        live = c['nonpadding'].sum(1)
        assert len(set(live.tolist())) == B and float(live.min()) > 0                         # ragged
        assert float(c['uv'][1].min()) == 1.0 and float(np_v[1].sum()) == 0                   # one row entirely unvoiced ...
        assert all(float(np_v[b].sum()) > 0 for b in range(B) if b != 1)                      # ... and no other row without a voiced frame
        assert sorted(c['pred'][:, :8, 1].flatten().tolist())[0] == -40.0 and float(c['pred'][:, :8, 1].max()) == 40.0
        if B * T > E.F0_FWD_FRAMES:                                                           # the frames of the second pass carry weight
            assert float(c['nonpadding'].flatten()[E.F0_FWD_FRAMES:].sum()) > 1000
    assert E.f0_case(10, 2000, 3)['pred'].shape == (10, 2000, 3)


def test_affine_shapes():
    n4 = [B * C * E.fs_ts(T) // 4 for B, C, T, _ in E.AFFINE_SHAPES]
    one_pass = E.EW_BLOCKS * 256                                                              # float4s one pass of the capped ew_grid covers
    assert one_pass == 4194304 and n4[2] == 4210688 > one_pass and max(n4[:2]) < one_pass
    assert E.fs_ts(64) == 64 and E.AFFINE_SHAPES[0][3] is None


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. the bound catches the bugs it is for
# ----------------------------------------------------------------------------------------------------------------------------------------
def _bn_seen(bug, B, T, kind):
    return {'first8192': B * E.fs_ts(T) > 4 * E.BN_STAGE4, 'ts_cols': T != E.fs_ts(T), 'e2': kind == 'cancellation'}[bug]


@pytest.mark.parametrize('B,T', E.BN_SHAPES + E.BN_SMALL)
@pytest.mark.parametrize('kind', E.BN_KINDS)
def test_batch_norm_bugs_exceed_the_bound(B, T, kind):
    c, want, ref = E.bn_refs(B, T, kind)
    for bug in ('first8192', 'ts_cols', 'e2'):
        dt = F32 if bug == 'e2' else F64                     # E[x^2] - E[x]^2 is wrong in float32 only
        ratio = E.worst_ratio(E.bn_restated(*_bn_args(c), dt, bug=bug), want, ref)
        print(f'bn[{B}x{T} {kind}] {bug}: {ratio:.3g} x the bound')
        if _bn_seen(bug, B, T, kind):
            assert ratio >= 100, (bug, ratio)
        elif bug != 'e2':
            assert ratio <= 1e-6, (bug, ratio)               # not observable: the formula is the right one here
    got = E.bn_restated(*_bn_args(c), F64, bug='biased')
    ratio = E.worst_ratio(got, want, ref)
    rv_bound = PH.bound(PH.rel_err(ref['running_var'], want['running_var']))
    print(f'bn[{B}x{T} {kind}] biased: {ratio:.3g} x the bound (n = {B * T}, running_var bound {rv_bound:.1e})')
    assert all(PH.rel_err(got[k], want[k]) <= 1e-12 for k in want if k != 'running_var')
    # the two variances differ by var / n, so running_var by at most 1 / n of its largest value: 100 x the floor of the bound needs n < 5000
    assert ratio <= 1 / (B * T * PH.FLOOR)
    if (B, T) in E.BN_SMALL:
        assert ratio >= 100, ratio
    else:
        assert B * T > 1 / (100 * PH.FLOOR)


@pytest.mark.parametrize('B,C,G,T', E.GN_SHAPES + E.GN_SMALL)
def test_group_norm_bugs_exceed_the_bound(B, C, G, T):
    c, want, ref = E.gn_refs(B, C, G, T)
    for bug, seen in (('utt0', B > 1), ('wave0', C // G > 1)):
        ratio = E.worst_ratio(E.gn_backward_manual(c['x'], c['gamma'], c['beta'], c['dy'], G, F64, bug=bug), want, ref)
        print(f'gn[{B}x{C}/{G}x{T}] {bug}: {ratio:.3g} x the bound')
        if seen:
            assert ratio >= 100, (bug, ratio)
        else:
            assert ratio <= 1e-6, (bug, ratio)


@pytest.mark.parametrize('B,T', E.F0_SHAPES + [(3, 301)])
@pytest.mark.parametrize('pitch_loss,use_uv', [('l1', True), ('l2', False)])
def test_pitch_loss_bugs_exceed_the_bound(B, T, pitch_loss, use_uv):
    c, hp, want, ref = E.f0_refs(B, T, 2, pitch_loss, use_uv)
    args = (c['pred'], c['f0'], c['uv'], c['nonpadding'], hp)
    for bug, seen in (('drop65536', B * T > E.F0_FWD_FRAMES), ('all_frames', use_uv)):
        got = E.f0_restated(*args, F64, bug=bug)
        ratio = E.worst_ratio(got, want, ref)
        values = E.worst_ratio({k: v for k, v in got.items() if k != 'dpred'}, want, ref)
        print(f'f0_loss[{B}x{T} {pitch_loss} uv={use_uv}] {bug}: {ratio:.3g} x the bound, the loss values alone {values:.3g} x')
        if seen:
            assert ratio >= 100 and values >= 100, (bug, ratio, values)
        else:
            assert ratio <= 1e-6, (bug, ratio)
