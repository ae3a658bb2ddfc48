"""No GPU: the vocoder optimisers' host side (include/dsv.h, section "Vocoder optimisers"; diffsinger_amd/voc_optim.py) - the float64 restatement
against the reference's recorded run, the RAdam scalars and their branch switch, the workspace size, the refusals of the entry points and the
state_dict round trips."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from diffsinger_amd import _lib
from tests import voc_optim_helpers as OH

ENTRIES = ['dsv_mt_chunk_floats', 'dsv_mt_table_tensors', 'dsv_mt_table_chunks', 'dsv_mt_set_table_limit', 'dsv_mt_workspace_floats',
           'dsv_mt_grad_norm', 'dsv_radam_scalars', 'dsv_mt_radam_step', 'dsv_mt_adamw_step']


@pytest.fixture(scope='module')
def fixture():
    return OH.load_fixture()


def test_header_section_binding_and_exports():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsv.h')).read()
    assert 'Vocoder optimisers' in hdr
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r'\b%s\(' % name, hdr) and name in _lib.SYMBOLS_VOC and hasattr(lib, name), name
    assert sorted(s for s in _lib.SYMBOLS_VOC if s.startswith('dsv_mt_') or s == 'dsv_radam_scalars') == sorted(ENTRIES)
    import diffsinger_amd
    for name in ('MultiTensorOptimizer', 'RAdam', 'AdamW', 'pwg_optimizers', 'hifigan_training_step'):
        assert name in diffsinger_amd.__all__ and getattr(diffsinger_amd, name) is not None


def test_fixture_is_what_the_recipe_says(fixture):
    p0, grads, traj = fixture
    q0, qg = OH.inputs(OH.FIXTURE_SIZES, OH.FIXTURE_SEED)
    assert [t.numel() for t in p0] == list(OH.FIXTURE_SIZES) == [1, 3, 5, 64, 1027] and len(grads) == 8 and sorted(traj) == sorted(OH.SETTINGS)
    assert all(torch.equal(a, b) for a, b in zip(p0, q0)) and all(torch.equal(a, b) for ga, gb in zip(grads, qg) for a, b in zip(ga, gb))
    assert os.path.getsize(OH.FIXTURE) < 600 * 1000
    assert any(hp['weight_decay'] != 0 for hp in OH.SETTINGS.values()) and any(hp['weight_decay'] == 0 for hp in OH.SETTINGS.values())


@pytest.mark.parametrize('name', sorted(OH.SETTINGS))
def test_restatement_within_the_floor_of_the_reference(fixture, name):
    """float64 restatement against the reference's own float32 run: the floor alone, every tensor, every step, parameters and both moments"""
    p0, grads, traj = fixture
    t64 = OH.restate(OH.radam_update, p0, grads, OH.SETTINGS[name], torch.float64)
    worst = 0.0
    for s in range(OH.STEPS):
        for kind, ref, want in zip(('p', 'exp_avg', 'exp_avg_sq'), traj[name][s], t64[s]):
            for i, (x, x64) in enumerate(zip(ref, want)):
                err, fl = float((x.double() - x64).abs().max()), OH.floor(x64, s + 1)
                assert err <= fl, (kind, 'step', s + 1, 'tensor', i, err, fl)
                worst = max(worst, err / fl)
    print(f'{name}: the reference stays within {worst:.3f} of the floor')
    # ... and the inputs are no empty test: both branches move every tensor by >= 100 x the bound
    OH.check_not_empty(name, p0, t64, traj[name])
    # the restatement in float32 (the stand-in where there is no fixture) is as good as the reference's run
    OH.check_trajectory(name, OH.restate(OH.radam_update, p0, grads, OH.SETTINGS[name], torch.float32), t64, traj[name])


@pytest.mark.parametrize('beta2', [0.999, 0.99])
def test_radam_scalars_and_the_branch_switch(beta2):
    lib = _lib.load()
    out = (C.c_double * 3)()
    branch = []
    for step in range(1, 11):
        for beta1 in (0.9, 0.8):
            assert lib.dsv_radam_scalars(step, beta1, beta2, out) == 0
            n_sma, size, rect = OH.radam_scalars(step, beta1, beta2)
            assert out[0] == n_sma and out[1] == size and out[2] == (1.0 if rect else 0.0), (step, beta1, list(out), n_sma, size)
        branch.append(out[2])
        if step in (5, 6):
            want = {(0.999, 5): 4.996, (0.99, 5): 4.960, (0.999, 6): 5.994, (0.99, 6): 5.941}[(beta2, step)]
            assert abs(out[0] - want) < 6e-4, (step, out[0])
    assert branch == [0.0] * 5 + [1.0] * 5
    assert lib.dsv_radam_scalars(0, 0.9, beta2, out) == -1 and b'dsv_radam_scalars' in lib.dsd_last_error()
    assert lib.dsv_radam_scalars(1, 0.9, 1.0, out) == -1 and lib.dsv_radam_scalars(1, 0.9, beta2, None) == -1


def test_adamw_restatement_against_torch_on_the_cpu():
    sizes = (1, 3, 5, 64, 1027)
    p0, grads = OH.inputs(sizes, 77)
    for hp in (dict(lr=0.1, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0), dict(lr=0.1, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)):
        t64 = OH.restate(OH.adamw_update, p0, grads, hp, torch.float64)
        t32 = OH.restate(OH.adamw_update, p0, grads, hp, torch.float32)
        params = [torch.nn.Parameter(t.clone()) for t in p0]
        opt = torch.optim.AdamW(params, foreach=False, **hp)
        got = []
        for gs in grads:
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()
            got.append(([p.detach().clone() for p in params], [opt.state[p]['exp_avg'].clone() for p in params],
                        [opt.state[p]['exp_avg_sq'].clone() for p in params]))
        OH.check_trajectory('adamw', got, t64, t32)
        OH.check_not_empty('adamw', p0, t64, t32)


def test_workspace_floats():
    lib = _lib.load()
    c = lib.dsv_mt_chunk_floats()
    assert c % 1024 == 0 and 1 <= lib.dsv_mt_table_tensors() <= 255 and lib.dsv_mt_table_chunks() >= 1

    def ws(*n):
        return lib.dsv_mt_workspace_floats((C.c_int64 * len(n))(*n), len(n))
    assert ws(1) == 2 and ws(c) == 2 and ws(c + 1) == 4 and ws(1, 3, c - 1, c, c + 1, 2 * c + 3) == 2 * (1 + 1 + 1 + 1 + 2 + 3)
    assert ws(1 << 40) == 2 * ((1 << 40) // c)
    assert ws(0) == -1 and ws(5, -1) == -1 and ws((1 << 40) + 1) == -1
    assert lib.dsv_mt_workspace_floats(None, 1) == -1 and lib.dsv_mt_workspace_floats((C.c_int64 * 1)(1), 0) == -1


def test_table_limit_knob():
    lib = _lib.load()
    kt, kc = lib.dsv_mt_table_tensors(), lib.dsv_mt_table_chunks()
    try:
        assert lib.dsv_mt_set_table_limit(3, 2) == 0 and (lib.dsv_mt_table_tensors(), lib.dsv_mt_table_chunks()) == (3, 2)
        assert lib.dsv_mt_set_table_limit(kt + 1, 0) == -1 and b'dsv_mt_set_table_limit' in lib.dsd_last_error()
        assert lib.dsv_mt_set_table_limit(0, kc + 1) == -1 and lib.dsv_mt_set_table_limit(-1, 0) == -1
        assert (lib.dsv_mt_table_tensors(), lib.dsv_mt_table_chunks()) == (3, 2)
    finally:
        assert lib.dsv_mt_set_table_limit(0, 0) == 0
    assert (lib.dsv_mt_table_tensors(), lib.dsv_mt_table_chunks()) == (kt, kc)


def test_bad_arguments_are_refused_before_any_launch():
    """every refusal returns DSD_ERR_INVALID (-1) with a message that names the entry point; the pointers are never followed (no GPU here)"""
    lib = _lib.load()
    ok = (C.c_void_p * 2)(0x1000, 0x2004)                      # float-aligned addresses that nothing reads
    odd = (C.c_void_p * 2)(0x1000, 0x2002)
    null = (C.c_void_p * 2)(0x1000, 0)
    n = (C.c_int64 * 2)(5, 7)
    n0 = (C.c_int64 * 2)(5, 0)
    hyper = (0.1, 0.9, 0.999, 1e-6, 0.0, 1)
    for name in ('dsv_mt_radam_step', 'dsv_mt_adamw_step'):
        fn = getattr(lib, name)
        bad = [(None, ok, ok, ok, n, 2) + hyper, (ok, None, ok, ok, n, 2) + hyper, (ok, ok, None, ok, n, 2) + hyper, (ok, ok, ok, None, n, 2) + hyper,
               (ok, ok, ok, ok, None, 2) + hyper, (ok, ok, ok, ok, n, 0) + hyper, (ok, ok, ok, ok, n0, 2) + hyper,
               (odd, ok, ok, ok, n, 2) + hyper, (ok, odd, ok, ok, n, 2) + hyper, (ok, ok, null, ok, n, 2) + hyper, (ok, ok, ok, null, n, 2) + hyper,
               (ok, ok, ok, ok, n, 2, -0.1, 0.9, 0.999, 1e-6, 0.0, 1), (ok, ok, ok, ok, n, 2, 0.1, 1.0, 0.999, 1e-6, 0.0, 1),
               (ok, ok, ok, ok, n, 2, 0.1, 0.9, -0.1, 1e-6, 0.0, 1), (ok, ok, ok, ok, n, 2, 0.1, 0.9, 0.999, -1e-6, 0.0, 1),
               (ok, ok, ok, ok, n, 2, 0.1, 0.9, 0.999, 1e-6, -1.0, 1), (ok, ok, ok, ok, n, 2, 0.1, 0.9, 0.999, float('nan'), 0.0, 1),
               (ok, ok, ok, ok, n, 2, 0.1, 0.9, 0.999, 1e-6, 0.0, 0)]
        for args in bad:
            assert fn(*args, None, None) == -1, (name, args[4:])
            assert name.encode() in lib.dsd_last_error(), lib.dsd_last_error()
        assert fn(ok, ok, ok, ok, n, 2, *hyper, 0x3002, None) == -1 and b'gscale' in lib.dsd_last_error()
    g = lib.dsv_mt_grad_norm
    for args in [(None, n, 2, 1.0, 0x4000, 4, 0x5000), (ok, None, 2, 1.0, 0x4000, 4, 0x5000), (ok, n, 0, 1.0, 0x4000, 4, 0x5000),
                 (ok, n0, 2, 1.0, 0x4000, 4, 0x5000), (odd, n, 2, 1.0, 0x4000, 4, 0x5000), (null, n, 2, 1.0, 0x4000, 4, 0x5000),
                 (ok, n, 2, -1.0, 0x4000, 4, 0x5000), (ok, n, 2, float('nan'), 0x4000, 4, 0x5000), (ok, n, 2, 1.0, None, 4, 0x5000),
                 (ok, n, 2, 1.0, 0x4004, 4, 0x5000), (ok, n, 2, 1.0, 0x4000, 3, 0x5000), (ok, n, 2, 1.0, 0x4000, 4, None),
                 (ok, n, 2, 1.0, 0x4000, 4, 0x5002)]:
        assert g(*args, None) == -1, args[2:]
        assert b'dsv_mt_grad_norm' in lib.dsd_last_error(), lib.dsd_last_error()


def _filled(opt_cls, hp, sizes=(3, 5)):
    params = [torch.nn.Parameter(torch.arange(n, dtype=torch.float32) + 1) for n in sizes]
    return params, opt_cls(params, **hp)


def test_state_dict_round_trips():
    from diffsinger_amd import AdamW, MultiTensorOptimizer, RAdam
    hp = dict(lr=0.01, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
    # the reference RAdam's layout: step a Python int, exp_avg, exp_avg_sq; groups of lr, betas, eps, weight_decay
    params, opt = _filled(RAdam, hp)
    assert isinstance(opt, MultiTensorOptimizer) and isinstance(opt, torch.optim.Optimizer)
    assert set(opt.param_groups[0]) >= {'params', 'lr', 'betas', 'eps', 'weight_decay'}
    ref_layout = {'state': {0: {'step': 7, 'exp_avg': torch.full((3,), 0.5), 'exp_avg_sq': torch.full((3,), 0.25)},
                            1: {'step': 4, 'exp_avg': torch.full((5,), -0.5), 'exp_avg_sq': torch.full((5,), 2.0)}},
                  'param_groups': [dict(hp, lr=0.005, params=[0, 1])]}
    opt.load_state_dict(ref_layout)
    st = [opt.state[p] for p in params]
    assert [s['step'] for s in st] == [7, 4] and all(type(s['step']) is int for s in st)
    assert torch.equal(st[0]['exp_avg'], torch.full((3,), 0.5)) and torch.equal(st[1]['exp_avg_sq'], torch.full((5,), 2.0))
    assert opt.param_groups[0]['lr'] == 0.005 and tuple(opt.param_groups[0]['betas']) == (0.8, 0.99)
    sd = opt.state_dict()
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'} and sd['state'][0]['step'] == 7 and type(sd['state'][1]['step']) is int
    params2, opt2 = _filled(RAdam, hp)
    opt2.load_state_dict(sd)
    assert [opt2.state[p]['step'] for p in params2] == [7, 4] and torch.equal(opt2.state[params2[1]]['exp_avg'], st[1]['exp_avg'])
    # torch.optim.AdamW's: step a tensor
    tp = [torch.nn.Parameter(torch.arange(n, dtype=torch.float32) + 1) for n in (3, 5)]
    topt = torch.optim.AdamW(tp, **hp)
    for _ in range(3):
        for p in tp:
            p.grad = torch.ones_like(p)
        topt.step()
    tsd = topt.state_dict()
    assert isinstance(tsd['state'][0]['step'], torch.Tensor)
    params3, opt3 = _filled(AdamW, hp)
    opt3.load_state_dict(tsd)
    for p, q in zip(params3, tp):
        s = opt3.state[p]
        assert s['step'] == 3 and type(s['step']) is int and s['exp_avg'].dtype == torch.float32 and s['exp_avg'].is_contiguous()
        assert torch.equal(s['exp_avg'], topt.state[q]['exp_avg']) and torch.equal(s['exp_avg_sq'], topt.state[q]['exp_avg_sq'])
    # ... and back: torch's AdamW takes ours
    topt2 = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(n)) for n in (3, 5)], **hp)
    topt2.load_state_dict(opt3.state_dict())
    assert float(topt2.state[topt2.param_groups[0]['params'][0]]['step']) == 3.0
    # StepLR drives the groups as it does any Optimizer's
    sched = torch.optim.lr_scheduler.StepLR(opt3, step_size=2, gamma=0.5)
    lrs = []
    for _ in range(4):
        sched.step()
        lrs.append(opt3.param_groups[0]['lr'])
    assert lrs == [0.01, 0.005, 0.005, 0.0025]


def test_cpu_tensors_and_other_types_raise():
    from diffsinger_amd import AdamW, MultiTensorOptimizer, RAdam
    for cls in (RAdam, AdamW):
        params, opt = _filled(cls, dict(lr=0.1))
        for p in params:
            p.grad = torch.ones_like(p)
        before = [p.detach().clone() for p in params]
        with pytest.raises(RuntimeError, match='no CPU path'):
            opt.step()
        with pytest.raises(RuntimeError, match='no CPU path'):
            opt.clip_and_step(1.0)
        assert all(torch.equal(a, b) for a, b in zip(before, params)) and all(not opt.state[p] for p in params)
        # no gradient anywhere: nothing to do, nothing raised
        for p in params:
            p.grad = None
        opt.step()
        assert float(opt.clip_and_step(1.0)) == 0.0 and all(not opt.state[p] for p in params)
    with pytest.raises(TypeError):
        MultiTensorOptimizer([torch.nn.Parameter(torch.zeros(2))])
    with pytest.raises(ValueError, match='hyper-parameters'):
        RAdam([torch.nn.Parameter(torch.zeros(2))], betas=(0.9, 1.0))
    half = torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))
    half.grad = torch.ones(2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='float32'):
        RAdam([half]).step()


def test_pwg_optimizers_from_the_config_blocks():
    from diffsinger_amd import RAdam, pwg_optimizers
    hp = dict(generator_optimizer_params=dict(lr=1e-4, eps=1e-6, weight_decay=0.0), generator_scheduler_params=dict(step_size=200000, gamma=0.5),
              discriminator_optimizer_params=dict(lr=5e-5, eps=1e-6, weight_decay=0.0), discriminator_scheduler_params=dict(step_size=3, gamma=0.5))
    gen, disc = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    gen.bias.requires_grad_(False)
    opt_g, opt_d, sched_g, sched_d = pwg_optimizers(gen, disc, hp)
    assert isinstance(opt_g, RAdam) and isinstance(opt_d, RAdam)
    assert opt_g.param_groups[0]['lr'] == 1e-4 and opt_g.param_groups[0]['eps'] == 1e-6 and tuple(opt_g.param_groups[0]['betas']) == (0.9, 0.999)
    assert [id(p) for p in opt_g.param_groups[0]['params']] == [id(gen.weight)] and len(opt_d.param_groups[0]['params']) == 2
    assert isinstance(sched_g, torch.optim.lr_scheduler.StepLR) and sched_g.step_size == 200000
    for _ in range(3):
        sched_d.step()
    assert opt_d.param_groups[0]['lr'] == 2.5e-5
