"""CPU: the host side of the ParallelWaveGAN discriminator (diffsinger_amd/pwg_disc.py, include/dsv.h section "PWG discriminator") - the module
tree has the reference's state-dict keys in every form a checkpoint can have, every unsupported configuration is refused in the constructor, the
float64 restatement the GPU tests measure against reproduces what the reference's own module computed (tests/golden/pwg_disc_ref.npz, written
by tools/make_golden_pwg_disc.py), and the C ABI is bound and exported."""
import inspect
import os

import pytest
import torch

from tests import pwg_disc_helpers as DH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pwg_disc_ref.npz')


@pytest.fixture(scope='module')
def fx():
    return DH.fixture()


def test_fixture_is_small_and_holds_the_four_layer_case(fx):
    assert os.path.getsize(GOLDEN) <= 300 * 1024
    assert fx['layers'] == 4 and fx['slope'] == 0.2
    assert tuple(fx['x'].shape) == tuple(fx['out'].shape) == tuple(fx['dx'].shape) == (2, 1, 1061)
    assert {k: tuple(v.shape) for k, v in fx['state'].items()} == DH.module_shapes(4)
    assert {k: tuple(v.shape) for k, v in fx['grads'].items()} == DH.module_shapes(4)
    assert sorted(fx['keys']) == ['wn0_b0', 'wn0_b1', 'wn1_b0', 'wn1_b1']


@pytest.mark.parametrize('wn', [True, False])
@pytest.mark.parametrize('bias', [True, False])
def test_constructor_keys_and_shapes_are_the_references(fx, wn, bias):
    from diffsinger_amd import ParallelWaveGANDiscriminator
    m = ParallelWaveGANDiscriminator(bias=bias, use_weight_norm=wn)
    want = [(k, tuple(s)) for k, s in fx['keys'][f'wn{int(wn)}_b{int(bias)}']]
    assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == sorted(want)
    assert dict(want) == DH.module_shapes(10, bias, wn)                      # the helper's restatement of the layout is the reference's too
    if wn:                                                                  # after remove_weight_norm(): the plain form
        m.remove_weight_norm()
        plain = [(k, tuple(s)) for k, s in fx['keys'][f'wn0_b{int(bias)}']]
        assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == sorted(plain)


def test_constructor_signature_is_the_references():
    from diffsinger_amd import ParallelWaveGANDiscriminator
    p = inspect.signature(ParallelWaveGANDiscriminator.__init__).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:]] == [
        ('in_channels', 1), ('out_channels', 1), ('kernel_size', 3), ('layers', 10), ('conv_channels', 64), ('dilation_factor', 1),
        ('nonlinear_activation', 'LeakyReLU'), ('nonlinear_activation_params', {'negative_slope': 0.2}), ('bias', True), ('use_weight_norm', True)]


def test_fixture_state_loads_strictly_and_a_plain_state_loads_into_a_weight_normed_module(fx):
    from diffsinger_amd import ParallelWaveGANDiscriminator
    m = ParallelWaveGANDiscriminator(layers=4)
    m.load_state_dict(fx['state'], strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, fx['state'][k]), k
    ws, bs = DH.plain_params(fx['state'], 4)
    plain = {}
    for i in range(4):
        plain[f'conv_layers.{2 * i}.weight'] = ws[i].float()
        plain[f'conv_layers.{2 * i}.bias'] = bs[i].float()
    m2 = ParallelWaveGANDiscriminator(layers=4, use_weight_norm=True)
    m2.load_state_dict(plain, strict=True)
    assert sorted(m2.state_dict()) == sorted(plain)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, plain[k]), k


@pytest.mark.parametrize('kw', [dict(layers=2), dict(layers=11), dict(conv_channels=32), dict(kernel_size=5), dict(dilation_factor=2),
                                dict(nonlinear_activation='ReLU', nonlinear_activation_params={}),
                                dict(nonlinear_activation_params={'negative_slope': 0.0}), dict(nonlinear_activation_params={'negative_slope': 1.0}),
                                dict(in_channels=2)], ids=lambda kw: ','.join(f'{k}={v}' for k, v in kw.items()))
def test_unsupported_configurations_are_refused_in_the_constructor(kw):
    from diffsinger_amd import ParallelWaveGANDiscriminator
    with pytest.raises(NotImplementedError, match='shipped configuration'):
        ParallelWaveGANDiscriminator(**kw)


def test_inputs_are_validated_before_any_device_work():
    from diffsinger_amd import ParallelWaveGANDiscriminator, lsgan_loss_op
    m = ParallelWaveGANDiscriminator(layers=3)
    for bad in (torch.zeros(2, 1, 8), torch.zeros(2, 1, 8, dtype=torch.float64), torch.zeros(2, 2, 8), torch.zeros(2, 8), torch.zeros(2, 1, 0)):
        with pytest.raises(ValueError, match='x must be'):
            m(bad)
    with pytest.raises(ValueError, match='d must be'):
        lsgan_loss_op(torch.zeros(4), 1.0)


def test_float64_restatement_reproduces_the_reference_module(fx):
    """The yardstick of the GPU tests pinned to the reference: forward64 / backward64 with their OWN masks against the recorded float32 CPU
    numbers, within the rule propagated layer by layer from x."""
    n, slope = fx['layers'], fx['slope']
    ws, bs = DH.plain_params(fx['state'], n)
    x = DH.d64(fx['x'])
    f = DH.forward64(x, ws, bs, slope)
    gp, e_gp = DH.generator_gp(f['p'], f['e_p'])
    bw = DH.backward64(gp, e_gp, x, ws, f['act'], slope, f['e_act'])
    rows = [('out', fx['out'], f['p'], f['e_p']), ('dx', fx['dx'], *bw['dx'])]
    for i in range(n):
        pre = f'conv_layers.{2 * i}.'
        (gg, bg), (gv, bv) = DH.weight_norm_grads64(DH.d64(fx['state'][pre + 'weight_g']), DH.d64(fx['state'][pre + 'weight_v']), *bw['dw'][i])
        rows += [(pre + 'weight_g', fx['grads'][pre + 'weight_g'], gg, bg), (pre + 'weight_v', fx['grads'][pre + 'weight_v'], gv, bv),
                 (pre + 'bias', fx['grads'][pre + 'bias'], *bw['db'][i])]
    for name, got, want, bound in rows:
        err = (DH.d64(got) - want).abs()
        k = int((err - bound).argmax())
        print(f'{name}: max err {float(err.max()):.3e}, at the tightest element err {float(err.flatten()[k]):.3e} <= bound {float(bound.flatten()[k]):.3e}')
        assert bool((err <= bound).all()), name


def test_helper_backward_is_the_autograd_of_its_forward():
    """backward64 with its own masks equals float64 autograd through forward64 (the restatement is self-consistent)."""
    shapes = DH.module_shapes(5, True, False)
    st = {k: v.double().requires_grad_(True) for k, v in DH.synth_state(shapes, 3).items()}
    ws = [st[f'conv_layers.{2 * i}.weight'] for i in range(5)]
    bs = [st[f'conv_layers.{2 * i}.bias'] for i in range(5)]
    x = torch.randn(2, 1, 53, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).requires_grad_(True)
    f = DH.forward64(x, ws, bs, 0.2)
    ((f['p'] - 1) ** 2).mean().backward()
    with torch.no_grad():
        gp, e_gp = DH.generator_gp(f['p'], None)
        bw = DH.backward64(gp, e_gp, x, ws, f['act'], 0.2)
        assert float((bw['dx'][0] - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
        for i in range(5):
            assert float((bw['dw'][i][0] - ws[i].grad).abs().max()) <= 1e-12 * float(ws[i].grad.abs().max()), i
            assert float((bw['db'][i][0] - bs[i].grad).abs().max()) <= 1e-12 * float(bs[i].grad.abs().max()), i


def test_public_names_and_symbols_are_exported():
    import diffsinger_amd
    from diffsinger_amd import _lib
    from tests.test_abi import _header_symbols
    for name in ('ParallelWaveGANDiscriminator', 'pwg_disc_op', 'lsgan_loss_op', 'generator_loss', 'discriminator_loss'):
        assert name in diffsinger_amd.__all__
        assert callable(getattr(diffsinger_amd, name))
    declared = [s for s in _header_symbols('dsv.h', 'dsv_') if s.startswith('dsv_pwgd_')]
    assert len(declared) == 13
    lib = _lib.load()
    for name in declared:
        assert name in _lib.SYMBOLS_VOC, name
        assert hasattr(lib, name), name
    assert lib.dsv_pwgd_tile() >= 32 and lib.dsv_pwgd_tile() % 32 == 0
    assert lib.dsv_pwgd_wgrad_split() >= 32 and lib.dsv_pwgd_wgrad_split() % 32 == 0
    S = lib.dsv_pwgd_wgrad_split()
    assert lib.dsv_pwgd_wgrad_workspace_floats(2, 2 * S + 37) == 2 * 3 * (64 * 64 * 3 + 64)
    for fn in (lib.dsv_pwgd_wgrad_workspace_floats, lib.dsv_pwgd_edge_workspace_floats):
        assert fn(0, 7) == -1 and fn(2, 0) == -1 and fn(65536, 7) == -1 and fn(2, -5) == -1
    assert lib.dsv_pwgd_lsgan_workspace_floats(0) == -1 and lib.dsv_pwgd_lsgan_workspace_floats(-3) == -1
    assert lib.dsv_pwgd_lsgan_workspace_floats(1) == 2
    # rejected before any HIP call, the message names the function
    assert lib.dsv_pwgd_layer(None, None, None, None, None, 1, 8, 1, 0.2, 0, None) == -1
    assert b'dsv_pwgd_layer' in lib.dsd_last_error()
    assert lib.dsv_pwgd_wgrad(None, None, None, None, None, 1, 8, 1, None) == -1
    assert b'dsv_pwgd_wgrad' in lib.dsd_last_error()
    assert lib.dsv_pwgd_lsgan(None, 1.0, None, None, 4, None) == -1
    assert b'dsv_pwgd_lsgan' in lib.dsd_last_error()
