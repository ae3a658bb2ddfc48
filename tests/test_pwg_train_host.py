"""CPU: ParallelWaveGAN generator training - the float64 restatement of tests/pwg_train_helpers.py against the reference's recorded numbers
(tests/golden/pwg_train_ref.npz, tools/make_golden_pwg_train.py), the C ABI's symbols and workspace queries, and everything forward_train
refuses before it asks for a device."""
import pytest
import torch

from tests import pwg_train_helpers as TH


@pytest.fixture(scope='module')
def fx():
    return TH.fixture()


@pytest.fixture(scope='module')
def restated(fx):
    return TH.module_grads(fx['state'], fx['x'], fx['c'], fx['cfg'], TH.mse_to(fx['target']))


def test_fixture_is_the_issue_configuration(fx):
    cfg = fx['cfg']
    assert (cfg['layers'], cfg['stacks'], cfg['aux'], cfg['scales'], cfg['ctx']) == (4, 2, 16, [4, 4, 4, 4], 2)
    assert tuple(fx['x'].shape) == (2, 1, 1536) and tuple(fx['c'].shape) == (2, 16, 10) and tuple(fx['out'].shape) == (2, 1, 1536)
    assert set(fx['state']) == set(TH.module_shapes(cfg))
    assert set(fx['grads']) | set(fx['none_keys']) == set(fx['state']) and not set(fx['grads']) & set(fx['none_keys'])
    for k, v in fx['state'].items():
        assert v.dtype == torch.float32 and bool((v.half().float() == v).all()), k          # stored as float16 without loss
    # the reference's own float32 against its float64: what the margin of 4 is taken on
    worst = max(fx['err'][k] / float(fx['grads'][k].abs().max()) for k in fx['err'] if k != 'first_conv.weight_v')
    print(f'reference float32 vs float64: output {fx["err_out"]:.2e}, gradients {worst:.2e} of max-abs')
    assert worst < 1e-4 and fx['err_out'] < 1e-6


def test_restatement_reproduces_the_reference_output(fx, restated):
    out = restated[0]
    err = float((out - fx['out'].double()).abs().max())
    tol = max(4 * fx['err_out'], TH.RULE * float(out.abs().max()))
    print(f'output: max err {err:.3e} <= {tol:.3e}')
    assert err <= tol


def test_restatement_reproduces_every_reference_gradient(fx, restated):
    _, grads, dw = restated
    tol = TH.tolerances(fx['state'], grads, dw, fx['err'])
    assert set(tol) == set(fx['grads'])
    for k in sorted(tol):
        err = float((grads[k] - fx['grads'][k].double()).abs().max())
        print(f'{k}: max err {err:.3e} <= {tol[k]:.3e} (4 x err_ref32 = {4 * fx["err"][k]:.3e}, max |grad| {float(grads[k].abs().max()):.3e})')
        assert err <= tol[k], k


def test_none_gradients_match_the_reference(fx, restated):
    none = sorted(k for k, g in restated[1].items() if g is None)
    assert none == sorted(fx['none_keys'])
    assert none == ['conv_layers.3.conv1x1_out.bias', 'conv_layers.3.conv1x1_out.weight_g', 'conv_layers.3.conv1x1_out.weight_v']


def test_first_conv_weight_v_gradient_is_zero_up_to_the_weight_norm_rule(fx, restated):
    """one element per row: d(g v / |v|) / dv = 0.  The tolerance of such a tensor comes from sum|term| of the expression, not from its size."""
    _, grads, dw = restated
    g = grads['first_conv.weight_v']
    _, bv = TH.weight_norm_bounds(TH.d64(fx['state']['first_conv.weight_g']), TH.d64(fx['state']['first_conv.weight_v']), dw['first_conv.'])
    assert float(g.abs().max()) < 1e-15 * float(dw['first_conv.'].abs().max())
    assert bool((fx['grads']['first_conv.weight_v'].double().abs() <= bv).all())


def test_gate_error_constant_is_derived():
    """A self-check of the helper (it passes without the product code): E_GATE is a few float32 roundings of values <= 1, and it holds on points
    its own grid did not see - a fresh seeded sample of the kernel's float32 formulas over [-GATE_RANGE, GATE_RANGE] stays within half of it (the
    other half is the margin for the device exponential).  Outside that range nothing is claimed: the GPU tests assert their pre-activations
    lie inside."""
    import numpy as np
    assert 1e-7 < TH.E_GATE < 2e-6
    f32 = np.float32
    rng = np.random.RandomState(7)
    a, g = (rng.uniform(-TH.GATE_RANGE, TH.GATE_RANGE, 200000).astype(f32) for _ in range(2))
    th, sg = f32(1) - f32(2) / (np.exp(f32(2) * a) + f32(1)), f32(1) / (f32(1) + np.exp(-g))
    th64, sg64 = np.tanh(a.astype(np.float64)), 1.0 / (1.0 + np.exp(-g.astype(np.float64)))
    for got, want in ((th, th64), (sg, sg64), (th * sg, th64 * sg64), (sg * (f32(1) - th * th), sg64 * (1 - th64 * th64)),
                      (th * (sg * (f32(1) - sg)), th64 * sg64 * (1 - sg64))):
        assert got.dtype == f32 and float(np.abs(got - want).max()) <= 0.5 * TH.E_GATE


def test_operator_restatements_are_the_autograd_of_the_block():
    """A self-check of the helper (it passes without the product code): gate_backward + conv_backward + wgrad_* equal float64 autograd through
    block(), so the explicit formulas the GPU operator tests compare the kernels with are the gradients of the forward they restate."""
    gen = torch.Generator().manual_seed(5)
    B, L, aux, dil = 2, 37, 8, 4
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)             # noqa: E731
    h, cond = r(B, 64, L).requires_grad_(True), r(B, aux, L).requires_grad_(True)
    ps = [r(128, 64, 3) / 14, r(128) * 0.1, r(128, aux, 1) / 3, r(64, 64, 1) / 8, r(64) * 0.1, r(64, 64, 1) / 8, r(64) * 0.1]
    for p in ps:
        p.requires_grad_(True)
    a, z, xo, sk = TH.block(h, cond, *ps, dil)
    dxp, dS = r(B, 64, L), r(B, 64, L)
    ((xo * dxp).sum() + (sk * dS).sum()).backward()
    with torch.no_grad():
        da, _ = TH.gate_backward(dxp, dS, a, ps[3], ps[5])
        (dx, _), (dc, _) = TH.conv_backward(da, dxp, ps[0], ps[2], dil)
        (dw1, _), (db1, _) = TH.wgrad_conv(da, h, cond, dil)
        (dw2, _), (db2, _) = TH.wgrad_out(dxp, dS, a)
        close = lambda u, v: float((u - v).abs().max()) <= 1e-12 * float(v.abs().max())    # noqa: E731
        assert close(dx, h.grad) and close(dc, cond.grad)
        assert close(dw1[:, :192].reshape(128, 3, 64).permute(0, 2, 1), ps[0].grad) and close(dw1[:, 192:, None], ps[2].grad) and close(db1, ps[1].grad)
        assert close(dw2[:64, :, None], ps[3].grad) and close(dw2[64:, :, None], ps[5].grad)
        assert close(db2[:64], ps[4].grad) and close(db2[64:], ps[6].grad)


def test_header_symbols_are_bound_and_exported_and_workspaces_consistent():
    import diffsinger_amd
    from diffsinger_amd import _lib
    from tests.test_abi import _header_symbols
    for name in ('pwg_gen_op', 'pwg_generator_losses', 'pwg_discriminator_losses', 'pwg_training_step'):
        assert name in diffsinger_amd.__all__ and callable(getattr(diffsinger_amd, name))
    declared = [s for s in _header_symbols('dsv.h', 'dsv_') if s.startswith('dsv_pwgt_')]
    assert len(declared) == 14
    lib = _lib.load()
    for name in declared:
        assert name in _lib.SYMBOLS_VOC, name
        assert hasattr(lib, name), name
    S = lib.dsv_pwgt_wgrad_split()
    assert S >= 32 and S % 32 == 0
    q = lib.dsv_pwgt_wgrad_workspace_floats
    assert q(2, 2 * S + 37, 272) == 2 * 3 * (128 * 272 + 128)
    assert q(1, S, 64) == 128 * 64 + 128 and q(1, S + 1, 64) == 2 * (128 * 64 + 128)
    assert q(3, 7, 192 + 128) == 3 * (128 * 320 + 128)
    assert q(0, 7, 64) == -1 and q(2, 0, 64) == -1 and q(65536, 7, 64) == -1 and q(2, 7, 0) == -1 and q(2, 7, 321) == -1 and q(2, 7, 60) == -1
    u = lib.dsv_pwgt_upsample_workspace_floats
    assert u(400, 4) == 2 * 400 * 9 and u(1, 1) == 6
    assert u(0, 4) == -1 and u(65536, 4) == -1 and u(4, 0) == -1 and u(4, 65) == -1
    # rejected before any HIP call, the message names the function
    assert lib.dsv_pwgt_layer(None, None, None, None, None, None, None, None, None, 1, 8, 0, 1, 1, None) == -1
    assert b'dsv_pwgt_layer' in lib.dsd_last_error()
    assert lib.dsv_pwgt_gate_backward(None, None, None, None, None, 1, 8, None) == -1
    assert b'dsv_pwgt_gate_backward' in lib.dsd_last_error()
    assert lib.dsv_pwgt_conv_backward(None, None, None, None, None, None, 1, 8, 0, 1, 1, None) == -1
    assert b'dsv_pwgt_conv_backward' in lib.dsd_last_error()
    assert lib.dsv_pwgt_wgrad_conv(None, None, None, None, None, 1, 8, 0, 1, None) == -1
    assert lib.dsv_pwgt_upsample_backward(None, None, None, None, None, None, 1, 8, 4, None) == -1
    assert b'dsv_pwgt_upsample_backward' in lib.dsd_last_error()


def _small(**kw):
    from diffsinger_amd.pwg import ParallelWaveGANGenerator
    args = dict(layers=2, stacks=1, aux_channels=8)
    args.update(kw)
    return ParallelWaveGANGenerator(**args)


def test_forward_train_refuses_what_it_does_not_cover_without_a_device():
    x, c = torch.zeros(1, 1, 256), torch.zeros(1, 8, 5)
    with pytest.raises(NotImplementedError, match='use_pitch_embed'):
        _small(use_pitch_embed=True).forward_train(x, c)
    with pytest.raises(NotImplementedError, match='dropout'):
        _small(dropout=0.05).forward_train(x, c)
    with pytest.raises(NotImplementedError, match='gradient'):
        _small().forward_train(x.clone().requires_grad_(True), c)
    with pytest.raises(NotImplementedError, match='gradient'):
        _small().forward_train(x, c.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match='conditioning'):
        _small().forward_train(x, None)
    with pytest.raises(ValueError, match='forward_train'):
        _small().forward_train(x[:, 0], c)
    with pytest.raises(ValueError, match='forward_train'):
        _small().forward_train(x, torch.zeros(1, 16, 5))
    with pytest.raises(RuntimeError, match='device'):
        _small().forward_train(x, c)                                             # host tensors: there is no CPU path
    for bad in (dict(kernel_size=5), dict(residual_channels=32), dict(aux_channels=12), dict(use_causal_conv=True)):
        with pytest.raises(NotImplementedError):
            _small(**bad)


def test_parameter_order_covers_every_parameter_in_both_forms():
    m = _small()
    ps = m._train_params()
    assert len(ps) == 3 + 4 + 7 * 2 + 4
    n_leaf = sum(1 for _ in m.parameters())
    assert n_leaf == len(TH.module_shapes(TH.config(layers=2, stacks=1, aux=8)))
    assert {k for k, _ in m.named_parameters()} == set(TH.module_shapes(TH.config(layers=2, stacks=1, aux=8)))
    m.remove_weight_norm()
    assert {k for k, _ in m.named_parameters()} == set(TH.module_shapes(TH.config(layers=2, stacks=1, aux=8), weight_norm_on=False))
    assert len(m._train_params()) == len(ps)
