"""The conditions of tests/fs2_ops_helpers.py judged on the CPU, before the GPU tests rely on them: they accept what is right (the float32
torch restatement, a float32 emulation of k_fs_attn's loop, aten's float32 convolution, a strictly sequential float32 chain) with room to
spare, and reject what is wrong (a padded key taken as live, a live key taken as dead, a raised reference maximum without the rescale).  The
emulation's counters are the evidence that the GPU cases reach the branches they are there for: raises of the lazy reference maximum after a
wave's first tile, and probabilities above 1 against an un-raised maximum.

Measured on the CPU: the float32 restatement uses at most 0.16 of the attention bound, the emulated kernel loop 0.17; the mask mutants exceed
it 5 000 to 13 000 times, the raise without the rescale 12 000 to 89 000 times; the bound itself is 1.5e-5 to 4.2e-4 of max|O|; aten's
convolution uses at most 0.25 and the sequential chain 0.27 of RULE sum|term| on these seeds."""
import functools

import pytest
import torch

from tests import fs2_ops_helpers as OH

ROOMY = ((3, 129), (3, 520))


@functools.lru_cache(maxsize=None)
def _case(kind, B, T):
    qkv, pad = OH.attention_inputs(kind, B, T, OH.seed_of(T))
    o64, bnd = OH.attention64(qkv, pad, 2)
    return qkv, pad, o64, bnd


@functools.lru_cache(maxsize=None)
def _emulated(kind, B, T):
    qkv, pad, _, _ = _case(kind, B, T)
    return OH.emulate_attention(qkv, pad, 2)


@pytest.mark.parametrize('B,T', OH.SHAPES)
@pytest.mark.parametrize('kind', OH.KINDS)
def test_attention_bound_accepts_the_float32_restatement(kind, B, T):
    qkv, pad, o64, bnd = _case(kind, B, T)
    assert bool(torch.isfinite(o64).all()) and bool(torch.isfinite(bnd).all()) and float(bnd.min()) >= 0
    o32 = OH.attention_ref(qkv, pad, 2, torch.float32)[0]
    share = OH.used(o32, o64, bnd)
    print(f'{kind} B={B} T={T}: fp32 CPU uses {share:.3f} of the bound; bound <= {float(bnd.max() / o64.abs().max()):.1e} max|O|')
    assert share <= 0.5


@pytest.mark.parametrize('B,T', ROOMY)
def test_attention_bound_rejects_a_wrong_key_mask(B, T):
    qkv, pad, o64, bnd = _case('flat', B, T)
    assert bool(pad[2, 37]) and not bool(pad[0, T - 1])
    live = pad.clone()
    live[2, 37] = False                                         # padded key 37 of utterance 2 taken as live
    dead = pad.clone()
    dead[0, T - 1] = True                                       # key T - 1 of utterance 0 taken as dead
    for name, mutant in (('padded key live', live), ('live key dead', dead)):
        o = OH.attention_ref(qkv, mutant, 2, torch.float64)[0]
        over = OH.used(o, o64, bnd)
        print(f'flat B={B} T={T} {name}: {over:.0f} x the bound')
        assert over >= 100


@pytest.mark.parametrize('B,T', OH.SHAPES)
@pytest.mark.parametrize('kind', OH.KINDS)
def test_emulated_kernel_loop_is_inside_the_bound(kind, B, T):
    _, _, o64, bnd = _case(kind, B, T)
    got, late, above = _emulated(kind, B, T)
    share = OH.used(got, o64, bnd)
    print(f'{kind} B={B} T={T}: emulated loop uses {share:.3f} of the bound; {late} late raises, {above} P > 1')
    assert share <= 1.0


def test_the_cases_reach_the_lazy_rescale_branches():
    assert _emulated('flat', 3, 129)[1] == 0                    # what the suite had: the raise after the first tile never taken
    for kind in ('ramp_up_fast', 'ramp_up_slow'):
        late = _emulated(kind, 3, 520)[1]
        print(f'{kind} (3, 520): {late} raises after a first tile')
        assert late >= 1000
    above = _emulated('ramp_up_slow', 3, 520)[2]
    print(f'ramp_up_slow (3, 520): {above} P > 1')
    assert above >= 100000


@pytest.mark.parametrize('B,T', [(3, 257), (3, 520), (1, 1030)])
def test_a_raise_without_the_rescale_is_rejected(B, T):
    qkv, pad, o64, bnd = _case('ramp_up_fast', B, T)
    got = OH.emulate_attention(qkv, pad, 2, drop_rescale=True)[0]
    over = OH.used(got, o64, bnd)
    print(f'ramp_up_fast B={B} T={T}: alpha = 1 on a raise is {over:.0f} x the bound')
    assert over > 1.0


@pytest.mark.parametrize('case', OH.CONV_CASES, ids=lambda c: 'B{}T{}Ci{}Co{}K{}d{}'.format(*c[:6]))
def test_conv_bound_accepts_float32_in_two_summation_orders(case):
    a = OH.conv_inputs(*case)
    y64, bnd = OH.conv64(a['x'], a['w'], a['b'], a['dil'], a['scale'], a['act'], a['res'], a['keep'])
    pre64 = OH.conv64(a['x'], a['w'], a['b'], a['dil'], 1.0, 'none', None, None)[0]
    rule = OH.RULE * OH.conv_sabs64(a['x'], a['w'], a['b'], a['dil'])
    for name, pre in (('aten', OH.conv32(a['x'], a['w'], a['b'], a['dil'])), ('sequential', OH.conv32_sequential(a['x'], a['w'], a['b'], a['dil']))):
        y = OH.conv_finish(pre, a['scale'], a['act'], a['res'], a['keep'])
        s_pre, s_y = OH.used(pre, pre64, rule), OH.used(y, y64, bnd)
        print(f'{case[:6]} {name}: contraction uses {s_pre:.3f} of RULE sum|term|, output {s_y:.3f} of the bound')
        assert s_pre <= 0.5 and s_y <= 1.0
    keep = a['keep']
    if keep is not None:
        assert float(bnd[keep == 0].abs().max()) == 0 and float(y64[keep == 0].abs().max()) == 0
