"""GPU: the vocoder optimisers (include/dsv.h, section "Vocoder optimisers"; diffsinger_amd/voc_optim.py) - RAdam and AdamW over lists of tensors
against the reference's recorded run and the float64 restatement, every alignment, skipped parameters, the launch seam, the global norm and its
clip coefficient, clip_and_step, and the two training steps that use them.  One bound everywhere: tests/voc_optim_helpers.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from diffsinger_amd import _lib
from tests import voc_optim_helpers as OH

pytestmark = pytest.mark.gpu

DEV = 'cuda'
UPDATES = {'RAdam': OH.radam_update, 'AdamW': OH.adamw_update}
ENTRY = {'RAdam': 'dsv_mt_radam_step', 'AdamW': 'dsv_mt_adamw_step'}
HPS = [dict(lr=0.1, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0), dict(lr=0.1, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)]

# The norm's floor, from the reduction of csrc/voc_optim.hpp.  A thread sums at most chunk / 256 = 64 squares in float32, in order: every term
# passes its own square's rounding and at most 63 additions (the first lands on 0 exactly) = 64 roundings of 2^-24 relative each, and all terms
# are >= 0, so the thread's sum is within 64 * 2^-24 of its true value.  The tree over the 256 threads, the partial per chunk and the sum of the
# partials are float64 (depth 0 in float32 terms, 2^-53 each: nothing).  So the sum of squares is within (64 + 0) * 2^-24; the square root
# halves that, and rounding the float64 root to float32 adds 2^-24 whole: (serial terms 64 + tree depth 0 + 2) * 2^-24 / 2 = 33 * 2^-24.
NORM_FLOOR = (64 + 0 + 2) * 2.0 ** -24 / 2


def lib():
    return _lib.load()


def chunk():
    return lib().dsv_mt_chunk_floats()


def seam_sizes():
    c = chunk()
    return [1, 3, 4, 5, 63, 64, 65, 1027, c - 1, c, c + 1, 2 * c + 3]


def many_small():
    return [1 + i % 7 for i in range(lib().dsv_mt_table_tensors() + 1)]         # K + 1 tensors of 1-7 elements: crosses the launch seam


def view_at(t, offset):
    """a device copy of t that starts `offset` floats into its storage"""
    base = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    v = base[offset:offset + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * offset) % 16
    return v


def run_optimizer(kind, p0, grads, hp, p_off=None, g_off=None, clip=None):
    """8 (or len(grads)) steps through the Optimizer -> per step (p, m, v) lists on the CPU.  grads[s][i] None: no gradient for tensor i."""
    import diffsinger_amd
    n = len(p0)
    params = [torch.nn.Parameter(view_at(t, p_off[i] if p_off else 0)) for i, t in enumerate(p0)]
    opt = getattr(diffsinger_amd, kind)(params, **hp)
    out = []
    for gs in grads:
        for i, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if g is None else view_at(g, g_off[i] if g_off else 0)
        if clip is None:
            opt.step()
        else:
            opt.clip_and_step(clip)
        zero = [torch.zeros_like(t) for t in p0]
        out.append(([p.detach().cpu() for p in params],
                    [opt.state[p]['exp_avg'].cpu() if opt.state[p] else zero[i] for i, p in enumerate(params)],
                    [opt.state[p]['exp_avg_sq'].cpu() if opt.state[p] else zero[i] for i, p in enumerate(params)]))
    return out, opt, params


def abi_step(kind, ps, gs, ms, vs, hp, step, gscale=None):
    k = len(ps)
    arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
    n = (C.c_int64 * k)(*[t.numel() for t in ps])
    _lib.call(ENTRY[kind], torch.device(DEV, torch.cuda.current_device()), arr(ps), arr(gs), arr(ms), arr(vs), n, k, hp['lr'], hp['betas'][0],
              hp['betas'][1], hp['eps'], hp['weight_decay'], step, _lib.ptr(gscale))


def grad_norm(gs, max_norm):
    k = len(gs)
    g = (C.c_void_p * k)(*[t.data_ptr() for t in gs])
    n = (C.c_int64 * k)(*[t.numel() for t in gs])
    nws = lib().dsv_mt_workspace_floats(n, k)
    ws = torch.full((nws // 2,), float('nan'), device=DEV, dtype=torch.float64)
    out2 = torch.full((2,), float('nan'), device=DEV)
    _lib.call('dsv_mt_grad_norm', torch.device(DEV, torch.cuda.current_device()), g, n, k, float(max_norm), ws.data_ptr(), nws, out2.data_ptr())
    return out2


def same_bits(a, b):
    return all(torch.equal(x, y) for sa, sb in zip(a, b) for la, lb in zip(sa, sb) for x, y in zip(la, lb))


# ---- 1. the reference's recorded run --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture():
    return OH.load_fixture()


@pytest.mark.parametrize('name', sorted(OH.SETTINGS))
def test_radam_against_the_reference_fixture(fixture, name):
    p0, grads, traj = fixture
    hp = OH.SETTINGS[name]
    t64 = OH.restate(OH.radam_update, p0, grads, hp, torch.float64)
    OH.check_not_empty(name, p0, t64, traj[name])
    got, opt, params = run_optimizer('RAdam', p0, grads, hp)
    worst = OH.check_trajectory(name, got, t64, traj[name])
    print(f'RAdam {name}: largest error / bound over 8 steps {worst:.3f}')
    assert all(opt.state[p]['step'] == 8 and type(opt.state[p]['step']) is int for p in params)


def test_adamw_on_the_fixture_inputs(fixture):
    p0, grads, _ = fixture
    for hp in HPS:
        t64 = OH.restate(OH.adamw_update, p0, grads, hp, torch.float64)
        t32 = OH.restate(OH.adamw_update, p0, grads, hp, torch.float32)
        OH.check_not_empty('adamw', p0, t64, t32)
        got, _, _ = run_optimizer('AdamW', p0, grads, hp)
        print(f'AdamW {hp["betas"]}: largest error / bound over 8 steps {OH.check_trajectory("adamw", got, t64, t32):.3f}')


# ---- 2. sizes around the vector width, the chunk and the table ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cases():
    """name -> (p0, grads): computed once, never modified"""
    return {'seams': OH.inputs(seam_sizes(), 31), 'many': OH.inputs(many_small(), 32)}


@pytest.fixture(scope='module')
def restated(cases):
    out = {}
    for (name, (p0, grads)), kind, (h, hp) in itertools.product(cases.items(), UPDATES, enumerate(HPS)):
        out[name, kind, h] = (OH.restate(UPDATES[kind], p0, grads, hp, torch.float64), OH.restate(UPDATES[kind], p0, grads, hp, torch.float32))
    return out


@pytest.mark.parametrize('h', [0, 1])
@pytest.mark.parametrize('kind', ['RAdam', 'AdamW'])
@pytest.mark.parametrize('name', ['seams', 'many'])
def test_sizes_against_the_restatement(cases, restated, name, kind, h):
    p0, grads = cases[name]
    t64, t32 = restated[name, kind, h]
    OH.check_not_empty(name, p0, t64, t32)
    got, _, _ = run_optimizer(kind, p0, grads, HPS[h])
    print(f'{kind} {name} setting {h}: largest error / bound {OH.check_trajectory(name, got, t64, t32):.3f}')
    again, _, _ = run_optimizer(kind, p0, grads, HPS[h])
    assert same_bits(got, again)                                            # two runs are bitwise equal
    if name == 'many':                                                      # the same list under tables of 5 tensors / 3 chunks: the same bits
        try:
            assert lib().dsv_mt_set_table_limit(5, 3) == 0
            split, _, _ = run_optimizer(kind, p0, grads, HPS[h])
        finally:
            assert lib().dsv_mt_set_table_limit(0, 0) == 0
        assert same_bits(got, split)


@pytest.mark.parametrize('kind', ['RAdam', 'AdamW'])
def test_a_tensor_that_continues_in_the_next_launch(cases, restated, kind):
    """chunk tables of 2 entries: the 3-chunk tensor of 'seams' is split over two launches, and the tensors behind it start new tables"""
    p0, grads = cases['seams']
    t64, t32 = restated['seams', kind, 1]
    whole, _, _ = run_optimizer(kind, p0, grads[:2], HPS[1])
    try:
        assert lib().dsv_mt_set_table_limit(0, 2) == 0
        split, _, _ = run_optimizer(kind, p0, grads[:2], HPS[1])
    finally:
        assert lib().dsv_mt_set_table_limit(0, 0) == 0
    assert same_bits(whole, split)
    OH.check_trajectory('split', split, t64[:2], t32[:2])


# ---- 3. alignment, skipped parameters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['RAdam', 'AdamW'])
def test_every_alignment_of_p_and_g(kind):
    offs = list(itertools.product(range(4), range(4)))                        # p and g independently at storage offsets 0..3 floats
    sizes = [(5, 1027, chunk() + 1)[i % 3] for i in range(len(offs))]
    p0, grads = OH.inputs(sizes, 33)
    hp = HPS[1]
    t64, t32 = OH.restate(UPDATES[kind], p0, grads, hp, torch.float64), OH.restate(UPDATES[kind], p0, grads, hp, torch.float32)
    got, _, _ = run_optimizer(kind, p0, grads, hp, p_off=[o[0] for o in offs], g_off=[o[1] for o in offs])
    OH.check_trajectory('aligned', got, t64, t32)
    # the vector path and the scalar path run the same arithmetic: the bits do not depend on where a tensor lies
    plain, _, _ = run_optimizer(kind, p0, grads, hp)
    assert same_bits(got, plain)


@pytest.mark.parametrize('kind', ['RAdam', 'AdamW'])
def test_moments_at_odd_offsets_and_gscale_through_the_abi(kind):
    sizes = [5, 1027, chunk() + 1, 64]
    p0, grads = OH.inputs(sizes, 34)
    hp = HPS[1]
    for gscale in (None, 0.37):
        gs_dev = None if gscale is None else torch.tensor([float('nan'), gscale], device=DEV)[1:]
        g32 = None if gscale is None else float(np.float32(gscale))
        t64 = OH.restate(UPDATES[kind], p0, grads, hp, torch.float64, gscale=g32)
        t32 = OH.restate(UPDATES[kind], p0, grads, hp, torch.float32, gscale=g32)
        OH.check_not_empty('gscale', p0, t64, t32)
        ps = [view_at(t, (0, 1, 2, 3)[i]) for i, t in enumerate(p0)]
        ms = [view_at(torch.zeros_like(t), (1, 0, 3, 2)[i]) for i, t in enumerate(p0)]
        vs = [view_at(torch.zeros_like(t), (3, 2, 0, 1)[i]) for i, t in enumerate(p0)]
        got = []
        for s, gl in enumerate(grads):
            abi_step(kind, ps, [view_at(g, (2, 3, 1, 0)[i]) for i, g in enumerate(gl)], ms, vs, hp, s + 1, gs_dev)
            got.append(([t.cpu() for t in ps], [t.cpu() for t in ms], [t.cpu() for t in vs]))
        print(f'{kind} gscale {gscale}: largest error / bound {OH.check_trajectory("abi", got, t64, t32):.3f}')


@pytest.mark.parametrize('kind', ['RAdam', 'AdamW'])
def test_parameters_without_a_gradient_are_skipped(kind):
    import diffsinger_amd
    sizes = [65, 7, 1027]
    p0, grads = OH.inputs(sizes, 35)
    hp = HPS[0]
    # the middle tensor never has a gradient: untouched, no state; its neighbours are right
    none_mid = [[g if i != 1 else None for i, g in enumerate(gs)] for gs in grads]
    t64, t32 = OH.restate(UPDATES[kind], p0, none_mid, hp, torch.float64), OH.restate(UPDATES[kind], p0, none_mid, hp, torch.float32)
    got, opt, params = run_optimizer(kind, p0, none_mid, hp)
    OH.check_trajectory('skipped', got, t64, t32)
    assert torch.equal(got[-1][0][1], p0[1]) and not opt.state[params[1]] and opt.state[params[0]]['step'] == 8
    # ... it joins at step 4 and sits out step 6: its own count lags, and one step() then serves two (group, step) buckets
    late = [[g if (i != 1 or s in (3, 4, 6, 7)) else None for i, g in enumerate(gs)] for s, gs in enumerate(grads)]
    t64, t32 = OH.restate(UPDATES[kind], p0, late, hp, torch.float64), OH.restate(UPDATES[kind], p0, late, hp, torch.float32)
    got, opt, params = run_optimizer(kind, p0, late, hp)
    OH.check_trajectory('late', got, t64, t32)
    assert [opt.state[p]['step'] for p in params] == [8, 4, 8]
    # a group with no gradient at all does nothing
    a, b = torch.nn.Parameter(p0[0].to(DEV)), torch.nn.Parameter(p0[2].to(DEV))
    opt = getattr(diffsinger_amd, kind)([dict(params=[a]), dict(params=[b], lr=0.5)], **hp)
    a.grad = grads[0][0].to(DEV)
    norm = opt.clip_and_step(1e9)
    assert torch.equal(b.detach().cpu(), p0[2]) and not opt.state[b] and opt.state[a]['step'] == 1 and not torch.equal(a.detach().cpu(), p0[0])
    assert abs(float(norm) / float(grads[0][0].double().norm()) - 1) < 1e-5
    a.grad = None
    before = a.detach().clone()
    opt.step()
    assert float(opt.clip_and_step(1.0)) == 0.0 and torch.equal(a.detach(), before) and opt.state[a]['step'] == 1


# ---- 4. the global norm --------------------------------------------------------------------------------------------------------------------------------
def norm_case(sizes, seed):
    _, grads = OH.inputs(sizes, seed, steps=1)
    gs = grads[0]
    n64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(params, gs):
        p.grad = g.clone()
    cpu = float(torch.nn.utils.clip_grad_norm_(params, float('inf')))
    return gs, n64, 4 * abs(cpu - n64) / n64 + NORM_FLOOR


@pytest.mark.parametrize('name', ['seams', 'many', 'one'])
def test_grad_norm_against_float64(name):
    sizes = {'seams': seam_sizes, 'many': many_small, 'one': lambda: [1]}[name]()
    gs, n64, bound = norm_case(sizes, 36)
    dev = [view_at(g, i % 4) for i, g in enumerate(gs)]
    for max_norm in (2.0 * n64, 0.25 * n64, float('inf'), 0.0):                 # one above the norm, one below
        out = grad_norm(dev, max_norm).cpu().numpy()
        rel = abs(float(out[0]) - n64) / n64
        print(f'{name}: norm {out[0]:.6e}, relative error {rel:.2e}, bound {bound:.2e}; max_norm {max_norm:.3e} -> coefficient {out[1]:.6f}')
        assert rel <= bound
        with np.errstate(over='ignore'):
            want = min(np.float32(1.0), np.float32(max_norm) / (out[0] + np.float32(1e-6)))
        assert out[1] == want and out[1].dtype == np.float32, (out[1], want)
        assert (out[1] == 1.0) == (max_norm > n64)
    # where the gradients lie does not change the bits, and neither does a second run
    aligned = [g.to(DEV) for g in gs]
    assert torch.equal(grad_norm(aligned, 1.0), grad_norm(dev, 1.0)) and torch.equal(grad_norm(dev, 1.0), grad_norm(dev, 1.0))
    # the same list in one table load and split over several: 3 tensors / 2 chunks per launch
    whole = grad_norm(dev, 1.0)
    try:
        assert lib().dsv_mt_set_table_limit(3, 2) == 0
        split = grad_norm(dev, 1.0)
    finally:
        assert lib().dsv_mt_set_table_limit(0, 0) == 0
    assert torch.equal(whole, split)


def test_a_non_finite_norm_propagates():
    gs = [torch.ones(5, device=DEV), torch.ones(1027, device=DEV)]
    gs[1][1000] = float('inf')
    out = grad_norm(gs, 1.0).cpu()
    assert float(out[0]) == float('inf') and float(out[1]) == 0.0               # torch: max_norm / (inf + 1e-6) = 0
    gs[1][1000] = float('nan')
    out = grad_norm(gs, 1.0).cpu()
    assert bool(torch.isnan(out).all())


# ---- 5. clip_and_step ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['RAdam', 'AdamW'])
def test_clip_and_step_is_the_norm_followed_by_the_scaled_step(kind):
    import diffsinger_amd
    sizes = [1, 5, 64, 1027, chunk() + 1]
    p0, grads = OH.inputs(sizes, 37)
    hp = HPS[1]
    params = [torch.nn.Parameter(t.to(DEV)) for t in p0]
    opt = getattr(diffsinger_amd, kind)(params, **hp)
    ps, ms, vs = [t.to(DEV) for t in p0], [torch.zeros_like(t, device=DEV) for t in p0], [torch.zeros_like(t, device=DEV) for t in p0]
    for s, gl in enumerate(grads):
        gd = [g.to(DEV) for g in gl]
        for p, g in zip(params, gd):
            p.grad = g.clone()
        n64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gl)))
        max_norm = 0.5 * n64 if s % 2 == 0 else 2.0 * n64                       # clipping on and off
        norm = opt.clip_and_step(max_norm)
        out2 = grad_norm(gd, max_norm)
        abi_step(kind, ps, gd, ms, vs, hp, s + 1, out2[1:])
        assert norm.dim() == 0 and norm.is_cuda and torch.equal(norm, out2[0]) and (float(out2[1]) < 1.0) == (s % 2 == 0)
        assert all(torch.equal(p.grad, g) for p, g in zip(params, gd))          # .grad is left unscaled
        for p, a, m, v in zip(params, ps, ms, vs):
            assert torch.equal(p.detach(), a) and torch.equal(opt.state[p]['exp_avg'], m) and torch.equal(opt.state[p]['exp_avg_sq'], v)
    # against the restatement with the coefficients the device formed: the clipped half of the steps really differs from the unclipped update
    unclipped, _, _ = run_optimizer(kind, p0, grads, hp)
    assert not torch.equal(unclipped[0][0][3], ps[3].cpu())


def test_a_strided_gradient_is_made_contiguous():
    from diffsinger_amd import RAdam
    p0 = torch.arange(12, dtype=torch.float32).reshape(3, 4) * 0.01
    g = (torch.arange(12, dtype=torch.float32).reshape(4, 3) - 5.0).t()         # not contiguous
    hp = HPS[0]
    p = torch.nn.Parameter(p0.to(DEV))
    p.grad = g.to(DEV)
    assert not p.grad.is_contiguous()
    RAdam([p], **hp).step()
    want = OH.restate(OH.radam_update, [p0], [[g.contiguous()]], hp, torch.float64)[0][0][0]
    ref = OH.restate(OH.radam_update, [p0], [[g.contiguous()]], hp, torch.float32)[0][0][0]
    assert float((p.detach().double().cpu() - want).abs().max()) <= OH.bound(want, ref, 1)
    half = torch.nn.Parameter(p0.to(DEV).half())
    half.grad = torch.ones_like(half)
    with pytest.raises(RuntimeError, match='float32'):
        RAdam([half], **hp).step()


# ---- 6. the ParallelWaveGAN step with its configured optimisers ---------------------------------------------------------------------------------------------
def _pwg_models():
    from diffsinger_amd import ParallelWaveGANDiscriminator
    from tests import pwg_disc_helpers as DH
    from tests import pwg_train_helpers as TH
    from tests.test_gpu_pwg_train import build
    f = TH.fixture()
    gen = build(f['cfg'], f['state'])
    disc = ParallelWaveGANDiscriminator(layers=10)
    disc.load_state_dict(DH.synth_state(DH.module_shapes(10), 41), strict=True)
    return gen, disc.to(DEV)


def test_pwg_training_step_with_the_configured_optimisers():
    from diffsinger_amd import MultiResolutionSTFTLoss, RAdam, pwg_optimizers, pwg_training_step
    from tests.test_gpu_pwg_train import rnd
    B, T = 2, 2560                                                           # the shape of tests/test_gpu_pwg_train.py's trainer
    batch = dict(x=rnd(B, 1, T, seed=42).to(DEV), c=rnd(B, 16, T // 256 + 4, seed=43).to(DEV), y=rnd(B, 1, T, seed=44, scale=0.3).to(DEV))
    stft = MultiResolutionSTFTLoss().to(DEV)
    # configs/tts/pwg.yaml's blocks, with a learning rate at which one step shows and a scheduler that halves after two
    hp = dict(lambda_adv=4.0, generator_grad_norm=1e-3, discriminator_grad_norm=1e-4, disc_start_steps=5,
              generator_optimizer_params=dict(lr=0.1, eps=1e-6, weight_decay=0.0), generator_scheduler_params=dict(step_size=2, gamma=0.5),
              discriminator_optimizer_params=dict(lr=0.05, eps=1e-6, weight_decay=0.0), discriminator_scheduler_params=dict(step_size=2, gamma=0.5))
    gen, disc = _pwg_models()
    gen2, disc2 = _pwg_models()
    # the clip norms: half of what this batch gives, so that clipping is active on both sides (no optimiser: nothing moves in this call)
    free = pwg_training_step(gen2, disc2, stft, batch, dict(hp, generator_grad_norm=1e9, discriminator_grad_norm=1e9), 5)
    hp.update(generator_grad_norm=0.5 * float(free['gen_grad_norm']), discriminator_grad_norm=0.5 * float(free['disc_grad_norm']))
    start ={0: [p.detach().double().cpu() for p in gen.parameters()], 1: [p.detach().double().cpu() for p in disc.parameters()]}
    opt_g, opt_d, sched_g, sched_d = pwg_optimizers(gen, disc, hp)
    out = pwg_training_step(gen, disc, stft, batch, hp, 5, opt_g, opt_d)
    grads = {0: [None if p.grad is None else p.grad.detach().double().cpu() for p in gen.parameters()],
             1: [None if p.grad is None else p.grad.detach().double().cpu() for p in disc.parameters()]}
    # the same step on a copy: clip_grad_norm_ (today's path with no optimiser), then step() of a second instance on the clipped gradients
    out2 = pwg_training_step(gen2, disc2, stft, batch, hp, 5)
    RAdam(list(gen2.parameters()), **hp['generator_optimizer_params']).step()
    RAdam(list(disc2.parameters()), **hp['discriminator_optimizer_params']).step()
    assert all(torch.equal(out[k], out2[k]) for k in out if not k.endswith('grad_norm')) and set(out) == set(out2)
    for side, (key, clip, block, m1, m2) in enumerate([('gen_grad_norm', 'generator_grad_norm', 'generator_optimizer_params', gen, gen2),
                                                       ('disc_grad_norm', 'discriminator_grad_norm', 'discriminator_optimizer_params', disc, disc2)]):
        n64 = float(torch.sqrt(sum((g ** 2).sum() for g in grads[side] if g is not None)))
        count = sum(g.numel() for g in grads[side] if g is not None)
        rel_torch = abs(float(out2[key]) - n64) / n64
        rel = abs(float(out[key]) - n64) / n64
        print(f'{key}: {float(out[key]):.6e} over {count} elements, relative error {rel:.2e} (torch on the device {rel_torch:.2e})')
        assert out[key].is_cuda and rel <= 4 * rel_torch + NORM_FLOOR and n64 > hp[clip]              # clipping is active
        coef = min(1.0, hp[clip] / (n64 + 1e-6))
        ohp = dict(betas=(0.9, 0.999), **hp[block])
        moved = 0.0
        for p0, g, p1, p2 in zip(start[side], grads[side], m1.parameters(), m2.parameters()):
            if g is None:
                assert torch.equal(p1.detach().double().cpu(), p0) and torch.equal(p2.detach().double().cpu(), p0)
                continue
            x64 = OH.restate(OH.radam_update, [p0.reshape(-1)], [[g.reshape(-1)]], ohp, torch.float64, gscale=coef)[0][0][0]
            b = OH.bound(x64, p2.detach().reshape(-1).cpu(), 1)
            err = float((p1.detach().reshape(-1).double().cpu() - x64).abs().max())
            assert err <= b, (key, tuple(p1.shape), err, b)
            moved = max(moved, float((x64 - p0.reshape(-1)).abs().max()) / b)
        assert moved >= 100, moved                                                                   # the step is visible at this learning rate
    # StepLR on the optimisers: halves at step_size
    sched_g.step(); sched_d.step()
    assert opt_g.param_groups[0]['lr'] == 0.1 and opt_d.param_groups[0]['lr'] == 0.05
    sched_g.step(); sched_d.step()
    assert opt_g.param_groups[0]['lr'] == 0.05 and opt_d.param_groups[0]['lr'] == 0.025
    # a torch optimiser and None take the path they took: clip_grad_norm_ scales .grad in place
    sgd = torch.optim.SGD(gen.parameters(), lr=0.0)
    other = pwg_training_step(gen, disc, stft, batch, dict(hp, generator_grad_norm=1e-3), 4, sgd)
    after = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in gen.parameters() if p.grad is not None)))
    assert float(other['gen_grad_norm']) > 1e-3 and abs(after / 1e-3 - 1) < 1e-3


# ---- 7. the HiFi-GAN step -----------------------------------------------------------------------------------------------------------------------------------
def test_hifigan_training_step():
    from diffsinger_amd import (AdamW, HifiGanMelLoss, MultiPeriodDiscriminator, hifigan_adversarial_losses, hifigan_discriminator_losses,
                                hifigan_generator_losses, hifigan_generator_step, hifigan_training_step)
    from diffsinger_amd.vocoder import HifiGanGenerator
    from tests import hifigan_train_helpers as TH
    from tests import mel_loss_helpers as MH
    fx = TH.fixture('plain')
    h = fx['h']
    gen = HifiGanGenerator(h)
    gen.load_state_dict(fx['state'], strict=True)
    gen = gen.to(DEV)
    B, T, hop = 2, 40, TH.hop_of(h)                                          # tests/test_gpu_mel_loss.py's generator step
    crit = HifiGanMelLoss(dict(fft_size=256, hop_size=hop, win_size=256, audio_num_mel_bins=40, fmin=0, fmax=12000, audio_sample_rate=24000)).to(DEV)
    batch = dict(x=torch.randn(B, 80, T, generator=torch.Generator().manual_seed(71)).to(DEV), y=MH.signals('near', T * hop, B)[1][:, None].to(DEV))
    torch.manual_seed(5)
    mpd = MultiPeriodDiscriminator().to(DEV)
    discs = [mpd]
    hp = dict(lambda_mel=45.0, adam_b1=0.8, adam_b2=0.99)
    gp, dp = [p for p in gen.parameters()], [p for p in mpd.parameters()]
    g0, d0 = [p.detach().clone() for p in gp], [p.detach().clone() for p in dp]
    out = hifigan_training_step(gen, discs, crit, batch, hp)
    g_dev = [None if p.grad is None else p.grad.clone() for p in gp]           # the generator objective's
    d_dev = [p.grad.clone() for p in dp]                                         # the discriminators' objective's
    assert all(torch.equal(a, b.detach()) for a, b in zip(g0 + d0, gp + dp))    # no optimiser: nothing moves
    # by hand, from the public operators
    for p in gp + dp:
        p.grad = None
    losses, y_hat = hifigan_generator_losses(gen, crit, batch['x'], None, batch['y'], lambda_mel=45.0)
    adv = hifigan_adversarial_losses(mpd, batch['y'], y_hat)
    total = losses['total'] + (adv['adv'] + adv['fm'])
    total.backward()
    assert torch.equal(out['gen_mel'], losses['mel'].detach()) and torch.equal(out['gen_adv'], adv['adv'].detach())
    assert torch.equal(out['gen_fm'], adv['fm'].detach()) and torch.equal(out['gen_total'], total.detach())
    assert all((a is None and p.grad is None) or torch.equal(a, p.grad) for a, p in zip(g_dev, gp))
    assert any(p.grad is not None for p in dp)                                   # the generator's terms reach the discriminator: the step drops them
    n64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g_dev if g is not None)))
    assert abs(float(out['gen_grad_norm']) / n64 - 1) < 1e-5
    for p in gp + dp:
        p.grad = None
    real, fake = hifigan_discriminator_losses(mpd, batch['y'], y_hat)
    (real + fake).backward()
    assert torch.equal(out['disc_real'], real.detach()) and torch.equal(out['disc_fake'], fake.detach()) and torch.equal(out['disc_total'], (real + fake).detach())
    assert all(p.grad is None for p in gp) and all(torch.equal(a, p.grad) for a, p in zip(d_dev, dp))
    # generator only: the discriminators are untouched; the mel-only step is what it was
    opt_g = AdamW(gp, lr=2e-4, betas=(hp['adam_b1'], hp['adam_b2']), weight_decay=0.0)
    hifigan_training_step(gen, discs, crit, batch, hp, opt_g=opt_g)
    assert all(torch.equal(a, p.detach()) for a, p in zip(d0, dp)) and any(not torch.equal(a, p.detach()) for a, p in zip(g0, gp))
    mel_only = hifigan_generator_step(gen, crit, batch, hp)
    assert set(mel_only) == {'gen_mel', 'gen_total', 'gen_grad_norm'} and all(torch.equal(a, p.detach()) for a, p in zip(d0, dp))
    # both optimisers: both sides step, the discriminators' side clipped at its norm
    opt_d = AdamW(dp, lr=2e-4, betas=(hp['adam_b1'], hp['adam_b2']), weight_decay=0.0)
    g1 = [p.detach().clone() for p in gp]
    both = hifigan_training_step(gen, discs, crit, batch, dict(hp, discriminator_grad_norm=1e-3), opt_g=opt_g, opt_d=opt_d)
    assert all(not torch.equal(a, p.detach()) for a, p in zip(d0, dp)) and any(not torch.equal(a, p.detach()) for a, p in zip(g1, gp))
    assert all(opt_d.state[p]['step'] == 1 for p in dp) and float(both['disc_grad_norm']) > 1e-3
    assert all(bool(torch.isfinite(p).all()) for p in gp + dp)
