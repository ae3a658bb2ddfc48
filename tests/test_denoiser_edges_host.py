"""CPU: the yardsticks of tests/test_gpu_denoiser_edges.py are what they claim to be, and the bound they set catches the bugs it is for.

  * `layer` / `forward` of tests/denoiser_edge_helpers.py are the oracle's residual layer / network: the same BITS in float32;
  * `wino_conv32` is the dilated convolution: equal to F.conv1d to 1e-12 in float64 for every length and dilation of the GPU tests; in float32
    its layer is no further from float64 than 4 x the direct form's (the two yardsticks differ little, so neither bound is the loose one);
  * three restated bugs - (a) the tail of y = x + step projection not zeroed behind T, (b) a tile's halo taken from the neighbouring utterance,
    (c) the left tap dropped across a tile boundary - exceed `tolerance` by at least 100 x at every length where they can be seen at all, are
    the exact convolution at every other length, and LENGTHS holds at least two visible lengths per bug and dilation."""
import pytest
import torch
import torch.nn.functional as F

from oracle import diffnet_oracle as O
from tests import denoiser_edge_helpers as E


def test_lengths_are_the_edge_set():
    assert E.LENGTHS == [1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 28, 30, 31, 32, 33, 34, 36, 40, 64, 65]
    assert set(E.SHORT) <= set(E.LENGTHS)
    for d in E.DILATIONS:
        assert any(T <= d for T in E.LENGTHS) and any(d < T <= 2 * d for T in E.LENGTHS)
        for name, (_, seen) in E.MUTANTS.items():
            assert sum(1 for T in E.LENGTHS if seen(T, d)) >= 2, (name, d)


@pytest.mark.parametrize('T', [1, 9, 33])
def test_layer_and_forward_are_the_oracle_bitwise_in_float32(T):
    cfg, p32, _, _ = E.model()
    inp = E.inputs(T)
    with torch.no_grad():
        d_emb = O.step_mlp(p32, cfg, inp['t'])
        for l in E.LAYERS:
            got, want = E.layer(p32, cfg, l, inp['x'], inp['cond'], d_emb), O.residual_layer(p32, cfg, l, inp['x'], inp['cond'], d_emb)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), l
        assert torch.equal(E.forward(p32, cfg, inp['spec'], inp['t'], inp['cond']), O.diffnet_forward(p32, cfg, inp['spec'], inp['t'], inp['cond']))
        # float64: the oracle's own function on a double copy of the parameters
        _, _, p64, _ = E.model()
        assert torch.equal(E.forward(p64, cfg, inp['spec'], inp['t'], inp['cond']),
                           O.diffnet_forward(p64, cfg, inp['spec'].double(), inp['t'], inp['cond'].double()))


@pytest.mark.parametrize('T', E.LENGTHS)
def test_winograd_restatement_is_the_convolution(T):
    """float64: F(2,3) == conv1d to 1e-12 (pairs that straddle T, taps that never meet the signal, every block count); the tile walk of the
    mutants with its switches off likewise.  float32: the Winograd layer against the direct layer, both against float64."""
    cfg, p32, p64, _ = E.model()
    inp = E.inputs(T)
    refs = E.layer_refs(T)
    for l, d in zip(E.LAYERS[:4], E.DILATIONS):
        w, b = p64[f'residual_layers.{l}.dilated_conv.weight'], p64[f'residual_layers.{l}.dilated_conv.bias']
        y = inp['x'].double()
        want = F.conv1d(y, w, b, padding=d, dilation=d)
        e_w = float((E.wino_conv32(y, w, b, d) - want).abs().max())
        e_t = float((E.tiled_conv(y, w, b, d) - want).abs().max())
        assert e_w <= 1e-12 and e_t <= 1e-12, (d, e_w, e_t)
        assert E.wino_conv32(inp['x'], w.float(), b.float(), d).dtype == torch.float32
        for i, name in enumerate(('x_out', 'skip')):
            ed, ew = E.maxerr(refs[l]['direct'][i], refs[l]['ref'][i]), E.maxerr(refs[l]['wino'][i], refs[l]['ref'][i])
            print(f'T={T} d={d} {name}: float32 direct {ed:.2e}, float32 Winograd {ew:.2e} ({ew / ed:.2f} x)')
            assert 0 < ew <= 4.0 * ed and ed <= 4.0 * ew, (d, name, ed, ew)
            assert E.tolerance('layer', refs[l]['ref'][i], refs[l]['direct'][i]) < 2e-5           # the reference sets the bound, not the cap


@pytest.mark.parametrize('T', E.LENGTHS)
def test_mutants_exceed_the_bound_where_they_are_observable(T):
    cfg, p32, p64, _ = E.model()
    inp = E.inputs(T)
    refs = E.layer_refs(T)
    with torch.no_grad():
        d_emb = O.step_mlp(p32, cfg, torch.full((E.B,), inp['t0']))
        for l, d in zip(E.LAYERS[:4], E.DILATIONS):
            bias = p64[f'residual_layers.{l}.output_projection.bias'][256:, None]
            for name, (conv, seen) in E.MUTANTS.items():
                xo, sk = E.layer(p64, cfg, l, inp['x'], inp['cond'], d_emb, conv=conv)
                worst = float('inf')
                for i, got in enumerate((xo, sk - bias)):
                    err = E.maxerr(got, refs[l]['ref'][i])
                    tol = max(E.tolerance('layer', refs[l]['ref'][i], refs[l][y][i]) for y in ('direct', 'wino'))
                    worst = min(worst, err / tol)
                    if not seen(T, d):
                        assert err <= 1e-12, (name, T, d, err)                  # not observable: the mutant IS the convolution here
                if seen(T, d):
                    print(f'T={T} d={d} mutant ({name}): {worst:.0f} x the bound')
                    assert worst >= 100.0, (name, T, d, worst)
