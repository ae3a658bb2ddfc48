"""CPU: the test side of HiFi-GAN generator training, ahead of the kernels (the training path itself is not built) - the
restatement a backward will be judged by (tests/hifigan_train_helpers.py) against the oracle, against the reference-generated fixture and against
torch's autograd."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hifigan_oracle as O
from tests import hifigan_train_helpers as TH


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(TH.FIXTURE) < (1 << 20)
    z = np.load(TH.FIXTURE, allow_pickle=False)
    assert {k.split('/')[0] for k in z.files} == set(TH.CASES)
    for k in z.files:
        assert z[k].dtype != object, k
    for case in TH.CASES:
        f = TH.fixture(case)
        assert f['h'] == TH.config(use_pitch_embed=case == 'nsf')
        assert {k: tuple(v.shape) for k, v in f['state'].items()} == TH.module_shapes(f['h'])
        assert all(torch.equal(v, v.half().float()) for v in f['state'].values())                  # the float16 state, without loss
        assert tuple(f['x'].shape) == (1, 80, 8) and tuple(f['out'].shape) == tuple(f['target'].shape) == (1, 1, 8 * TH.hop_of(f['h']))
        assert set(f['grads']) | set(f['none_keys']) == set(f['state']) and set(f['err']) == set(f['grads'])
        n = sum(m.numel() for m in f['masks'])
        print(f'{case}: seed {f["seed"]}, {len(f["masks"])} leaky ReLUs with {n} inputs, err_out {f["err_out"]:.2e}')
        assert len(f['masks']) == 1 + 4 * (3 * 6 + 1) and n == 68352
        assert (f['f0'] is not None) == (case == 'nsf') == (f['sine_waves'] is not None)
        if case == 'nsf':
            assert tuple(f['sine_waves'].shape) == (1, 8 * 64, 9) and bool((f['f0'] == 0).any()) and bool((f['f0'] > 0).any())


@pytest.mark.parametrize('resblock', ['1', '2'])
@pytest.mark.parametrize('nsf', [False, True])
def test_restatement_is_bitwise_the_oracle_in_float32(nsf, resblock):
    h = TH.config(use_pitch_embed=nsf, resblock=resblock, upsample_initial_channel=16)
    p = O.synth_generator_params(h, 11)
    assert {k: tuple(v.shape) for k, v in p.items()} == TH.module_shapes(h, weight_norm_on=False)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 80, 5, generator=gen)
    f0 = None
    if nsf:
        f0 = 200.0 + 50.0 * torch.rand(2, 5, generator=gen)
        f0[0, 1:3] = 0.0
    torch.manual_seed(13)
    want = O.generator(p, h, x, f0)
    torch.manual_seed(13)
    got, pre, sw, har = TH.generator(p, h, x, f0)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    per = 6 if resblock == '1' else 2
    assert len(pre) == 1 + 4 * (3 * per + 1)
    # the same evaluation on its own masks and its own sine_waves: the same bits again (where() picks x or slope x exactly as leaky_relu does)
    again, _, _, _ = TH.generator(p, h, x, f0, masks=TH.masks_of(pre), sine_waves=sw)
    assert torch.equal(again, want)
    # a weight-normed state goes through the oracle's own weight-norm op
    st = TH.synth_state(TH.module_shapes(h), 14)
    torch.manual_seed(15)
    want = O.generator(st, h, x, f0)
    torch.manual_seed(15)
    assert torch.equal(TH.generator(TH.plain_weights(st, h), h, x, f0)[0], want)


@pytest.mark.parametrize('case', TH.CASES)
def test_float64_on_the_recorded_masks_reproduces_the_fixture(case):
    f = TH.fixture(case)
    out, g64, dw64, pre, _ = TH.module_grads(f['state'], f['h'], f['x'], f['f0'], TH.mse_to(f['target']), masks=f['masks'], sine_waves=f['sine_waves'])
    e = float((out - f['out'].double()).abs().max())
    print(f'output: max err {e:.3e} (4 x err_out = {4 * f["err_out"]:.3e})')
    assert e <= max(4 * f['err_out'], TH.RULE * float(out.abs().max()))
    flips, n = TH.count_flips(TH.masks_of(pre), f['masks'])
    print(f'float64 against the recorded float32 masks: {flips} of {n} differ')
    assert flips == 0                                                                            # the tool refuses a seed for which they differ
    assert sorted(k for k, g in g64.items() if g is None) == sorted(f['none_keys'])
    tol = TH.tolerances(f['state'], g64, dw64, f['err'])
    worst = 0.0
    for k in sorted(tol):
        err = float((f['grads'][k].double() - g64[k]).abs().max())
        bound = min(tol[k], 4 * f['err'][k] + TH.RULE * float(g64[k].abs().max()))
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
    print(f'{len(tol)} gradients, worst err / bound {worst:.2f}')


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('Co,Ci,K,dil,slope', [(5, 3, 3, 1, 0.1), (4, 6, 7, 3, 0.1), (1, 4, 7, 1, 0.01), (3, 2, 11, 5, 1.0)])
def test_convolution_operator_functions_agree_with_autograd(Co, Ci, K, dil, slope):
    B, L = 2, 37
    pad = TH.get_padding(K, dil)
    x, w, g = _rand(B, Ci, L, seed=1).requires_grad_(True), _rand(Co, Ci, K, seed=2).requires_grad_(True), _rand(B, Co, L, seed=3)
    x.data[0, 0, 5] = 0.0                                                  # a zero takes the slope
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    F.conv1d(F.leaky_relu(x, slope), w, b, padding=pad, dilation=dil).backward(g)
    close = lambda u, v: float((u - v).abs().max()) <= 1e-12 * max(float(v.abs().max()), 1e-30)    # noqa: E731
    (dw, bw), (db, bb) = TH.conv_wgrad(g, x.detach(), K, dil, pad, slope)
    assert close(dw, w.grad) and close(db, b.grad) and bool((bw >= 0).all()) and bool((bb > 0).all())
    res, acc = _rand(B, Ci, L, seed=4), _rand(B, Ci, L, seed=5)
    dx, bx = TH.conv_dgrad(g, w.detach(), x.detach(), dil, pad, slope)
    assert close(dx, x.grad) and bool((bx >= (TH.RULE * dx.abs()) * (1 - 1e-12)).all())
    dx2, _ = TH.conv_dgrad(g, w.detach(), x.detach(), dil, pad, slope, residual=res, sum_in=acc, divide=3.0)
    assert close(dx2, (x.grad + res + acc) / 3.0)


def test_source_operator_functions_agree_with_autograd():
    B, L, C, s = 2, 24, 3, 4
    har, w, g = torch.tanh(_rand(B, L, seed=9)), _rand(C, 2 * s, seed=10), _rand(B, C, L // s, seed=11)
    hr, wr = har.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv1d(hr[:, None], wr[:, None], bias, stride=s, padding=s // 2).backward(g)
    (dw, _), (db, _), (dh, _) = TH.noise_conv_backward(g, har, w, s, s // 2)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())               # noqa: E731
    assert close(dw, wr.grad) and close(db, bias.grad) and close(dh, hr.grad)
    sw, lw, lb = _rand(B, L, 9, seed=12), _rand(1, 9, seed=13).requires_grad_(True), _rand(1, seed=14).requires_grad_(True)
    hh = torch.tanh(F.linear(sw, lw, lb))[..., 0]
    hh.backward(dh)
    (dlw, _), (dlb, _) = TH.source_backward(dh, hh.detach(), sw)
    assert close(dlw, lw.grad[0]) and close(dlb, lb.grad)
