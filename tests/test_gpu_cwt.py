"""The CWT pitch path on the MI355X (csrc/fs2_cwt.hpp: k_cwt2f0, k_cwt2f0_bwd, k_cwt_loss_partial / _final / _bwd) through its public surface:
fs2.cwt2f0_op, FastSpeech2.cwt2f0_norm, losses.cwt_pitch_loss_terms and losses.fs2_losses, on the case tables of tests/cwt_helpers.py (what the
tables hold, and that the float64 yardstick is the reference's own arithmetic, is asserted on the CPU by tests/test_cwt_host.py).

Judgement, for every value and every gradient: the device's distance from the float64 restatement <= max(2 x e_ref, 4 x 2^-23 x max|reference|),
e_ref = the distance of the torch fp32 expression the operator replaces (FastSpeech2.cwt2f0_norm's expression, losses._add_pitch_loss's
expressions; on the device, same inputs) from the same restatement.  The floor covers the exp, the log2 and two roundings, the factor 2 a
different order of summation.  Every comparison prints the device's distance beside its allowance (`report`).  Two calls must agree bit for
bit, forward and backward; the uv channel of the 11-wide parent must receive exact zeros from cwt2f0_op.

NOT IN THE TABLES, because the reference itself is non-finite there (a division by a zero deviation): one live frame, and constant rows.

MEASURED on the MI355X, 2026-10-21: 26 tests in 6.2 s.  ratio = the device's distance / its allowance, worst over the family (passes at <= 1):
    FWD        out 0.131   d cwt 0.133 (random) 0.138 (tail)   d mean 0.111 / 0.114   d std 0.147 / 0.155          (183 cases, T = 2 ... 513)
    FIXTURE    forward: out 0.087 against the reference's own float64 results; loss terms <= 0.156, gradients <= 0.175
    LOSS       C 0.112   uv 0.159   f0_mean 0.130   f0_std 0.113   d cwt 0.172   d mean 0.036   d std 0.095            (31 cases)
    OBJECTIVE  fs2_losses with the f0 term: values <= 0.177, gradients <= 0.118
    E2E        fs2_lj_free with the fused route: mel_out 3.3e-6, f0_denorm 8.9e-7 relative (bounds 1e-4)"""
import contextlib

import pytest
import torch

from diffsinger_amd import fs2, losses
from tests import cwt_helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
FWD, LOSS = H.fwd_cases(), H.loss_cases()


def report(family, what, ratios):
    print(f'CWT {family} | {what} | ' + ' '.join(f'{k}={r:.3f} ({e:.1e}/{a:.1e})' for k, (r, e, a) in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v[0] <= 1.0}
    assert not bad, (what, bad)


def worst(acc, new):
    for k, v in new.items():
        if k not in acc or v[0] > acc[k][0]:
            acc[k] = v


@contextlib.contextmanager
def routes(infer=None, loss=None, glue=True):
    before = dict(fs2._CWT_NATIVE)
    try:
        fs2.set_cwt_native(infer=infer, loss=loss)
        fs2.set_glue(glue)
        yield
    finally:
        fs2.set_cwt_native(**before)
        fs2.set_glue(True)


# ---- cwt2f0_op: values and gradients --------------------------------------------------------------------------------------------------------
def _leaf_and_view(parent):
    leaf = parent.to(DEV).requires_grad_(True)
    return leaf, leaf[:, :, :10]


def _upstreams(c, seed):
    g = torch.Generator().manual_seed(seed)
    ups = {'random': torch.randn(c.B, c.T + c.pad, generator=g)}
    if c.pad:
        tail = torch.zeros(c.B, c.T + c.pad)
        tail[:, c.T:] = torch.randn(c.B, c.pad, generator=g)
        ups['tail'] = tail                                       # non-zero on the padded columns only: all of it lands on frame T - 1
    return ups


def run_fwd_case(c, o=None, want64=None):
    """the operator, today's fp32 expression (both on the device) and the float64 restatement (CPU) on one case -> {name: (ratio, err, allow)}"""
    o = o or H.fwd_operands(c)
    hp, T_out = H.HP_NORM[c.norm], c.T + c.pad
    plain = c.live == c.T and c.pad == 0                        # the reference's own call: no frame_keep
    m2p = o['mel2ph'].to(DEV)
    keep, live = fs2.frame_keep(m2p)
    assert int(live) == c.live
    res = {}

    def device(fn):
        leaf, view = _leaf_and_view(o['parent'])
        mean, std = o['mean'].to(DEV).requires_grad_(True), o['std'].to(DEV).requires_grad_(True)
        out = fn(view, mean, std)
        grads = {k: torch.autograd.grad(out, (leaf, mean, std), u.to(DEV), retain_graph=True) for k, u in _upstreams(c, 7).items()}
        return out.detach(), grads

    got, g_got = device(lambda v, m, s: fs2.cwt2f0_op(v, m, s, T_out, hp, std_scale=c.std_scale, live=None if plain else live))
    again, g_again = device(lambda v, m, s: fs2.cwt2f0_op(v, m, s, T_out, hp, std_scale=c.std_scale, live=None if plain else live))
    assert torch.equal(got, again), (c, 'two forward calls differ')
    for k in g_got:
        assert all(torch.equal(a, b) for a, b in zip(g_got[k], g_again[k])), (c, k, 'two backward calls differ')
    today, g_today = device(lambda v, m, s: H.cwt2f0_norm_today(v, m, s * c.std_scale, T_out, hp, fk=None if plain else (keep[:, :c.T], live)))

    p64 = o['parent'].double().requires_grad_(True)
    m64, s64 = o['mean'].double().requires_grad_(True), o['std'].double().requires_grad_(True)
    ref = H.cwt2f0_norm_ref(p64[:, :, :10], m64, s64, T_out, hp, c.std_scale, c.live)
    assert got.shape == ref.shape == (c.B, T_out) and bool(torch.isfinite(ref).all())
    res['out'] = H.error_rule(got.cpu(), ref.detach(), today.cpu())
    if want64 is not None:
        res['out_fixture'] = H.error_rule(got.cpu(), want64, today.cpu())
    frozen = H.cwt2f0_norm_ref(p64[:, :, :10], m64, s64, T_out, hp, c.std_scale, c.live, frozen_stats=True)
    for k, u in _upstreams(c, 7).items():
        g_ref = torch.autograd.grad(ref, (p64, m64, s64), u.double(), retain_graph=True)
        direct = torch.autograd.grad(frozen, p64, u.double(), retain_graph=True)[0]          # the terms that cancel in d cwt (error_rule)
        for name, a, b, t in zip(('dcwt', 'dmean', 'dstd'), g_got[k], g_ref, g_today[k]):
            assert a.shape == b.shape and bool(torch.isfinite(a).all())
            res[f'{name}_{k}'] = H.error_rule(a.cpu(), b, t.cpu(), cancelling=direct if name == 'dcwt' else None)
        if o['parent'].shape[2] == 11:
            assert float(g_got[k][0][:, :, 10].abs().max()) == 0.0, (c, 'the uv channel of the parent got a gradient')
    return res


@pytest.mark.parametrize('T', H.FWD_T)
def test_cwt2f0_values_and_gradients_on_the_table(T):
    acc = {}
    cases = [c for c in FWD if c.T == T]
    for c in cases:
        res = run_fwd_case(c)
        bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
        assert not bad, (c, bad)
        worst(acc, res)
    report('FWD', f'T={T}, {len(cases)} cases, worst of each', acc)


def test_cwt2f0_on_the_reference_fixture():
    g = H.load_golden()
    for i in range(len(H.GOLDEN_FWD)):
        c, o, want = H.golden_fwd(g, i)
        report('FIXTURE', f'forward {i} {tuple(c)}', run_fwd_case(c, o, want))


def test_reduction_order_depends_on_the_live_frames_only():
    """The forward over [B, n] equals, on its n columns, the forward over a longer allocation (and a longer T_out) whose statistics run over the
    same n frames - bit for bit, for n on both sides of the block size; and a strided view gives the bits of its contiguous copy."""
    hp = H.HP_NORM['log']
    g = torch.Generator().manual_seed(5)
    for n in (2, 65, H.BLOCK - 1, H.BLOCK, H.BLOCK + 1, 2 * H.BLOCK + 1):
        for extra, pad in ((1, 0), (37, 0), (37, 5), (H.BLOCK, 1)):
            B = 3
            long = torch.randn(B, n + extra, 11, generator=g).to(DEV)
            mean, std = torch.tensor(H.ROW_MEANS, device=DEV), (torch.rand(B, generator=g) * 0.5 + 0.1).to(DEV)
            live = torch.tensor(float(n), device=DEV)
            short = fs2.cwt2f0_op(long[:, :n, :10], mean, std, n, hp)
            budget = fs2.cwt2f0_op(long[:, :, :10], mean, std, n + extra + pad, hp, live=live)
            assert torch.equal(short, budget[:, :n]), (n, extra, pad)
            exact = fs2.cwt2f0_op(long[:, :, :10].contiguous(), mean, std, n + extra + pad, hp, std_scale=1.0, live=live)
            assert torch.equal(exact, budget), 'the strided view and its contiguous copy differ'


def test_cwt2f0_op_refuses_what_it_cannot_take():
    hp = H.HP_NORM['log']
    x, m, s = torch.randn(2, 5, 10, device=DEV), torch.zeros(2, device=DEV), torch.ones(2, device=DEV)
    with pytest.raises(RuntimeError, match='no CPU path'):
        fs2.cwt2f0_op(x.cpu(), m.cpu(), s.cpu(), 5, hp)
    with pytest.raises(TypeError, match='float32'):
        fs2.cwt2f0_op(x.double(), m, s, 5, hp)
    with pytest.raises(ValueError, match=r'\[B, T, 10\]'):
        fs2.cwt2f0_op(torch.randn(2, 5, 11, device=DEV), m, s, 5, hp)
    with pytest.raises(ValueError, match='T_out'):
        fs2.cwt2f0_op(x, m, s, 4, hp)
    with pytest.raises(ValueError, match='mean and std'):
        fs2.cwt2f0_op(x, m[:1], s, 5, hp)
    with pytest.raises(NotImplementedError):
        fs2.cwt2f0_op(x, m, s, 5, dict(pitch_norm='none'))


# ---- FastSpeech2.cwt2f0_norm: which route runs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', ['log', 'standard'])
def test_model_method_routes(norm):
    from diffsinger_amd import hparams
    from tests import fs2_helpers as FH
    case, m, hp, params, inp = FH.case_setup('fs2_lj_free')
    c = H.FwdCase(3, 65, 0, 64, 'view11', norm, 1.0)
    o = H.fwd_operands(c)
    saved = {k: hparams.get(k) for k in ('pitch_norm', 'f0_mean', 'f0_std')}
    try:
        hparams.update(H.HP_NORM[norm])
        parent, mean, std, m2p = o['parent'].to(DEV), o['mean'].to(DEV), o['std'].to(DEV), o['mel2ph'].to(DEV)
        view = parent[:, :, :10]
        for fk in (None, fs2.frame_keep(m2p)):
            with torch.no_grad():
                today = H.cwt2f0_norm_today(view, mean, std, c.T, H.HP_NORM[norm], fk=fk)
                op = fs2.cwt2f0_op(view, mean, std, c.T, H.HP_NORM[norm], live=fk[1] if fk is not None else None)
                with routes(infer=True):
                    assert torch.equal(m.cwt2f0_norm(view, mean, std, m2p, fk=fk), op), 'route on: not the bits of the operator'
                with routes(infer=True, glue=False):
                    assert torch.equal(m.cwt2f0_norm(view, mean, std, m2p, fk=fk), today), '_GLUE off: not the bits of the expression'
                with routes(infer=False):
                    assert torch.equal(m.cwt2f0_norm(view, mean, std, m2p, fk=fk), today), 'route off: not the bits of the expression'
        # a gradient is required: the operator, whatever the inference switch says; with _GLUE off the expression
        leaf = parent.clone().requires_grad_(True)
        with routes(infer=False):
            out = m.cwt2f0_norm(leaf[:, :, :10], mean, std, m2p)
            assert type(out.grad_fn).__name__.startswith('_Cwt2F0')
            assert torch.equal(out.detach(), fs2.cwt2f0_op(view, mean, std, c.T, H.HP_NORM[norm]))
        with routes(glue=False):
            assert not type(m.cwt2f0_norm(leaf[:, :, :10], mean, std, m2p).grad_fn).__name__.startswith('_Cwt2F0')
    finally:
        for k, v in saved.items():
            if v is None:
                hparams.pop(k, None)
            else:
                hparams[k] = v


def test_end_to_end_reference_case_with_the_fused_route_on():
    """fs2_lj_free, the reference-generated free-running cwt forward tests/test_gpu_fs2.py replays, with dsf_cwt2f0 in the forward: that
    file's bounds for f0_denorm and mel_out."""
    import numpy as np
    from tests import fs2_helpers as FH
    from tests.test_gpu_fs2 import _run_hip
    g = FH.load_golden('fs2_lj_free')
    with routes(infer=True):
        out = _run_hip('fs2_lj_free')
    np.testing.assert_array_equal(out['mel2ph'], g['mel2ph'])
    err = float(np.abs(out['mel_out'] - g['mel_out']).max())
    f = float((np.abs(out['f0_denorm'] - g['f0_denorm']) / np.maximum(np.abs(g['f0_denorm']), 1.0)).max())
    print(f'CWT E2E | fs2_lj_free, fused route | mel_out max-abs err {err:.3e} (bound 1e-4)  f0_denorm rel err {f:.3e} (bound 1e-4)')
    assert out['mel_out'].shape == g['mel_out'].shape and err <= 1e-4
    assert f <= 1e-4


# ---- the loss terms --------------------------------------------------------------------------------------------------------------------------
W = (1.0, 0.5, 2.0, 1.5)                 # upstream weights of C, uv, f0_mean, f0_std: no term hides behind another


def _loss_leaves(o, dtype, dev):
    """-> (leaf of the predictor's output, its view as the operator is given it, f0_mean_pred, f0_std_pred), each requiring grad"""
    v = o['cwt']
    base = v._base if v._base is not None else v
    leaf = base.detach().to(device=dev, dtype=dtype).clone().requires_grad_(True)
    view = leaf[:, :, :v.shape[2]] if v._base is not None else leaf
    return leaf, view, o['f0_mean_pred'].to(device=dev, dtype=dtype).requires_grad_(True), o['f0_std_pred'].to(device=dev, dtype=dtype).requires_grad_(True)


def _sample(o, dtype, dev):
    return {k: (o[k].to(device=dev, dtype=dtype) if o[k].is_floating_point() else o[k].to(dev)) for k in ('cwt_spec', 'uv', 'mel2ph', 'f0', 'f0_mean', 'f0_std')}


def _weighted(L):
    keys = [k for k in ('C', 'uv', 'f0_mean', 'f0_std') if k in L]
    return sum(W[('C', 'uv', 'f0_mean', 'f0_std').index(k)] * L[k] for k in keys)


def run_loss_case(c, o=None, hp=None, want=None):
    o, hp = o or H.loss_operands(c), hp or H.loss_hp(c)
    res = {}

    def evaluate(dtype, dev, fused):
        leaf, view, mp, sp = _loss_leaves(o, dtype, dev)
        out, s = {'cwt': view, 'f0_mean': mp, 'f0_std': sp}, _sample(o, dtype, dev)
        if dev == 'cpu':
            L = H.pitch_loss_ref(out, s, hp)
        else:
            L = {}
            with routes(loss=fused):
                losses._add_pitch_loss(out, s, hp, L)
        grads = torch.autograd.grad(_weighted(L), (leaf, mp, sp))
        return {k: v.detach().cpu() for k, v in L.items()}, [g.cpu() for g in grads], leaf

    L_got, g_got, leaf = evaluate(F32, DEV, True)
    L_again, g_again, _ = evaluate(F32, DEV, True)
    assert list(L_got) == list(L_again) and all(torch.equal(L_got[k], L_again[k]) for k in L_got), (c, 'two forward calls differ')
    assert all(torch.equal(a, b) for a, b in zip(g_got, g_again)), (c, 'two backward calls differ')
    L_today, g_today, _ = evaluate(F32, DEV, False)
    L_ref, g_ref, _ = evaluate(F64, 'cpu', None)
    assert list(L_got) == list(L_ref) == list(L_today), (list(L_got), list(L_ref))
    for k in L_ref:
        res[k] = H.error_rule(L_got[k], L_ref[k], L_today[k])
        if want is not None:
            res[k + '_fixture'] = H.error_rule(L_got[k], want[k], L_today[k])
    for name, a, b, t in zip(('dcwt', 'dmean', 'dstd'), g_got, g_ref, g_today):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        res[name] = H.error_rule(a, b, t)
    wide = g_got[0]
    used = 11 if c.use_uv else 10
    if wide.shape[2] > used:
        assert float(wide[:, :, used:].abs().max()) == 0.0, (c, 'a channel behind the predictor\'s got a gradient')
    if c.use_uv:
        dead = (o['mel2ph'] == 0)
        assert float(wide[:, :, 10][dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, (c, 'a padding frame got a uv gradient')
    return res


SMALL = [c for c in LOSS if c.B * c.T <= 4 * H.BLOCK]
LARGE = [c for c in LOSS if c.B * c.T > 4 * H.BLOCK]


@pytest.mark.parametrize('loss', ['l1', 'l2'])
def test_loss_terms_on_the_table(loss):
    acc = {}
    cases = [c for c in SMALL if c.loss == loss]
    for c in cases:
        res = run_loss_case(c)
        bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
        assert not bad, (c, bad)
        worst(acc, res)
    report('LOSS', f'{loss}, {len(cases)} cases, worst of each', acc)


@pytest.mark.parametrize('c', LARGE, ids=lambda c: f'{c.B}x{c.T}-{c.loss}')
def test_loss_terms_where_the_grids_wrap(c):
    report('LOSS', f'{tuple(c)}', run_loss_case(c))


def test_loss_terms_on_the_reference_fixture():
    g = H.load_golden()
    for i in range(len(H.GOLDEN_LOSS)):
        c, hp, o, keys, vals = H.golden_loss(g, i)
        hp4 = dict(hp, cwt_add_f0_loss=False)                    # the four fused terms; the f0 term: test_fs2_losses_with_the_f0_term
        want = {k: v for k, v in zip(keys, vals) if k != 'f0'}
        report('FIXTURE', f'loss {i} {tuple(c)}', run_loss_case(c, o, hp4, want))


def test_loss_with_an_empty_mask_is_nan_like_the_expression():
    c = H.LossCase(2, 9, 'l1', True, 'view11', 'ragged')
    o = H.loss_operands(c)
    o['mel2ph'] = torch.zeros_like(o['mel2ph'])
    for fused in (True, False):
        L = {}
        with routes(loss=fused):
            losses._add_pitch_loss({'cwt': o['cwt'].to(DEV), 'f0_mean': o['f0_mean_pred'].to(DEV), 'f0_std': o['f0_std_pred'].to(DEV)}, _sample(o, F32, DEV),
                                   H.loss_hp(c), L)
        assert bool(torch.isnan(L['uv'])) and all(bool(torch.isfinite(L[k])) for k in ('C', 'f0_mean', 'f0_std')), (fused, L)


def test_cwt_pitch_loss_terms_refuses_what_it_cannot_take():
    c = H.LossCase(2, 9, 'l1', True, 'contig', 'ragged')
    o = {k: v.to(DEV) for k, v in H.loss_operands(c).items()}
    args = lambda **kw: [kw.get(k, o[k]) for k in ('cwt', 'cwt_spec', 'uv', 'mel2ph', 'f0_mean_pred', 'f0_mean', 'f0_std_pred', 'f0_std')]
    assert losses.cwt_pitch_loss_terms(*args()).shape == (4,)
    with pytest.raises(ValueError, match='no CPU path'):
        losses.cwt_pitch_loss_terms(*args(cwt=o['cwt'].cpu()))
    with pytest.raises(ValueError, match='float32'):
        losses.cwt_pitch_loss_terms(*args(cwt_spec=o['cwt_spec'].double()))
    with pytest.raises(ValueError, match='11'):
        losses.cwt_pitch_loss_terms(*args(cwt=o['cwt'][:, :, :10]))
    with pytest.raises(ValueError, match='shape'):
        losses.cwt_pitch_loss_terms(*args(uv=o['uv'][:, :-1]))
    with pytest.raises(NotImplementedError):
        losses.cwt_pitch_loss_terms(*args(), cwt_loss='ssim')


# ---- fs2_losses with the f0 term ----------------------------------------------------------------------------------------------------------------
def _objective(c, hp_extra):
    from tests import fs2_loss_edge_helpers as V
    from tests.test_gpu_fs2_loss import LOSS_HP
    Tt = 12
    hp = dict(LOSS_HP, mel_loss='ssim:0.5|l1:0.5', use_pitch_embed=True, use_energy_embed=False, lambda_ph_dur=0.7, lambda_word_dur=1.3, lambda_sent_dur=0.9)
    hp.update(H.loss_hp(c, **hp_extra))
    mel_out, mels = V.mel_operands(V.MelCase(c.B, c.T, 80, 6.0, 'tail', 'contig'))
    d = V.dur_operands(V.DurCase(c.B, Tt, c.T, 'sil', 'random'))
    o = H.loss_operands(c)
    o['mel2ph'] = d['mel2ph']
    o['f0'] = o['f0'] * 0 + (torch.rand(c.B, c.T, generator=torch.Generator().manual_seed(3)) * 2 + 8.5) * (d['mel2ph'] > 0)
    if hp['pitch_norm'] == 'standard':
        o['f0'] = (2 ** o['f0'] - hp['f0_mean']) / hp['f0_std'] * (d['mel2ph'] > 0)
    return hp, dict(mel_out=mel_out, dur=d['dur_pred']), dict(mels=mels, txt_tokens=d['tok']), o


@pytest.mark.parametrize('extra', [dict(pitch_loss='l1'), dict(pitch_loss='l2', pitch_norm='standard', f0_mean=214.0, f0_std=63.5)],
                         ids=['l1-log', 'l2-standard'])
def test_fs2_losses_with_the_f0_term(extra):
    """cwt_add_f0_loss with use_uv false: the reference's keys in its order, the restated objective's values, and its gradient at
    output['cwt'] / ['f0_mean'] / ['f0_std'] (the f0 term reaches them through dsf_cwt2f0_bwd)."""
    from tests.test_gpu_fs2_loss import SIL, _objective_reference
    c = H.LossCase(3, 33, 'l1', False, 'view11', 'ragged')
    hp, other, sample0, o = _objective(c, dict(extra, cwt_add_f0_loss=True))
    pitch_keys = ['C', 'f0_mean', 'f0_std', 'f0']

    def evaluate(dtype, dev, fn):
        leaf, view, mp, sp = _loss_leaves(o, dtype, dev)
        out = dict({k: v.to(device=dev, dtype=dtype) for k, v in other.items()}, cwt=view, f0_mean=mp, f0_std=sp)
        s = dict(_sample(o, dtype, dev), **{k: (v.to(device=dev, dtype=dtype) if v.is_floating_point() else v.to(dev)) for k, v in sample0.items()})
        L = fn(out, s)
        grads = torch.autograd.grad(sum(L[k] for k in pitch_keys), (leaf, mp, sp))
        return {k: v.detach().cpu() for k, v in L.items()}, [g.cpu() for g in grads]

    def restated(out, s):
        L = _objective_reference(out, s, dict(hp, use_pitch_embed=False), 'fs2')
        L.update(H.pitch_loss_ref(out, s, hp))
        return L

    L_got, g_got = evaluate(F32, DEV, lambda out, s: losses.fs2_losses(out, s, hp, variant='fs2', sil_ph_ids=list(SIL)))
    L_ref, g_ref = evaluate(F64, 'cpu', restated)
    L_32, g_32 = evaluate(F32, DEV, lambda out, s: dict(H.pitch_loss_ref(out, s, hp)))          # the fp32 yardstick of the pitch terms, on the device
    assert list(L_got) == list(L_ref) == ['ssim', 'l1', 'pdur', 'wdur', 'sdur'] + pitch_keys, list(L_got)
    for k in ('ssim', 'l1', 'pdur', 'wdur', 'sdur'):
        assert abs(float(L_got[k]) - float(L_ref[k])) <= 1e-5 * max(abs(float(L_ref[k])), 1e-3), k
    res = {k: H.error_rule(L_got[k], L_ref[k], L_32[k]) for k in pitch_keys}
    for name, a, b, t in zip(('dcwt', 'dmean', 'dstd'), g_got, g_ref, g_32):
        res[name] = H.error_rule(a, b, t)
    assert float(g_got[0][:, :, 10].abs().max()) == 0.0
    report('OBJECTIVE', f'fs2_losses, cwt_add_f0_loss, {extra}', res)


def test_fs2_losses_refuses_the_f0_term_with_use_uv():
    c = H.LossCase(3, 33, 'l1', True, 'contig', 'ragged')
    from tests.test_gpu_fs2_loss import SIL
    hp, other, sample0, o = _objective(c, dict(cwt_add_f0_loss=True))
    out = dict({k: v.to(DEV) for k, v in other.items()}, cwt=o['cwt'].to(DEV), f0_mean=o['f0_mean_pred'].to(DEV), f0_std=o['f0_std_pred'].to(DEV))
    s = dict(_sample(o, F32, DEV), **{k: v.to(DEV) for k, v in sample0.items()})
    with pytest.raises(ValueError, match=r'tasks/tts/fs2.py:257'):
        losses.fs2_losses(out, s, hp, variant='fs2', sil_ph_ids=list(SIL))
