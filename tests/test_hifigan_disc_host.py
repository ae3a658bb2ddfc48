"""CPU: the test infrastructure of the HiFi-GAN scale discriminator - the fixture recorded from the reference (tests/golden/hifigan_disc_ref.npz),
its keys and shapes, and the float64 restatement of tests/hifigan_disc_helpers.py against the recorded reference numbers - and the host side of
what diffsinger_amd/hifigan_disc.py holds (the pooling; checked on the GPU in tests/test_gpu_hifigan_disc.py)."""
import os

import numpy as np
import pytest
import torch

from diffsinger_amd import _lib
from tests import hifigan_disc_helpers as DH


@pytest.fixture(scope='module')
def fx():
    return DH.fixture()


@pytest.fixture(scope='module')
def inputs():
    return DH.fixture_inputs()


@pytest.fixture(scope='module')
def restated(inputs):
    """the float64 restatement in both modes, computed once: {mode: (forward, backward)}"""
    state, y, y_hat = inputs
    out = {}
    for mode in ('eval', 'train'):
        fw = DH.msd_forward64(state, y, y_hat, mode == 'train')
        out[mode] = (fw, DH.msd_backward64(fw, state, DH.FIXTURE_T))
    return out


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(DH.FIXTURE) <= 600 * 1000
    meta = fx['meta']
    assert (meta['B'], meta['T'], meta['seed'], meta['samples']) == (DH.FIXTURE_B, DH.FIXTURE_T, DH.FIXTURE_SEED, DH.FIXTURE_SAMPLES)
    assert len(meta['keys']) == 80 and len(meta['shapes']) == 80
    lens = [DH.lengths(t) for t in (300, 150, 75)]
    assert lens[0] == [300, 150, 75, 19, 5, 5, 5, 5] and DH.lengths(1061) == [1061, 531, 266, 67, 17, 17, 17, 17]
    for mode in ('eval', 'train'):
        assert fx[f'{mode}/losses'].shape == (4,) and fx[f'{mode}/dy_hat'].shape == (1, 1, 300)
        for i in range(3):
            assert fx[f'{mode}/r{i}'].shape == (1, lens[i][7]) and fx[f'{mode}/g{i}'].shape == (1, lens[i][7])
            for l in range(DH.N):
                n = min(DH.FIXTURE_SAMPLES, DH.LAYERS[l][1] * lens[i][l])
                assert fx[f'{mode}/fr{i}_{l}'].shape == (n,) == fx[f'idx/fg{i}_{l}'].shape
        for l in range(DH.N):
            assert fx[f'{mode}/u{l}'].shape == (DH.LAYERS[l][1],)
    grads = [k for k in fx if k.startswith('eval/grad/')]
    assert len(grads) == 64 and all(fx[k].size <= DH.FIXTURE_SAMPLES for k in grads)


def test_keys_and_shapes_are_the_references(fx, inputs):
    """the twin module and the restated shapes carry the reference's 80 state-dict entries; a strict load of the regenerated state succeeds"""
    twin = DH.TwinMSD()
    sd = twin.state_dict()
    assert list(sd) == fx['meta']['keys']
    assert [list(v.shape) for v in sd.values()] == fx['meta']['shapes']
    assert {k: tuple(v.shape) for k, v in sd.items()} == DH.module_shapes()
    assert sum(p.numel() for p in twin.discriminators[1].parameters()) == 9874306                  # 9.87 M, weight_g counted
    twin.load_state_dict(inputs[0], strict=True)


def test_inputs_are_validated_before_device_work():
    from diffsinger_amd import hifigan_disc as HD
    import diffsinger_amd
    assert diffsinger_amd.avg_pool_op is HD.avg_pool_op and diffsinger_amd.cond_discriminator_loss is HD.cond_discriminator_loss
    n0 = HD.launch_count()
    ok = torch.zeros(2, 1, 64)
    with pytest.raises(ValueError, match='no CPU path'):
        HD.avg_pool_op(ok)
    with pytest.raises(ValueError, match='float32'):
        HD.avg_pool_op(ok.double())
    with pytest.raises(ValueError, match=r'\[B\]\[1\]\[T\]'):
        HD.avg_pool_op(torch.zeros(2, 2, 64))
    with pytest.raises(ValueError, match='T >= 2'):
        HD.avg_pool_op(ok[:, :, :1])
    with pytest.raises(ValueError, match='no CPU path'):
        HD.cond_discriminator_loss([ok])
    assert HD.launch_count() == n0


def test_twin_module_is_the_functional_restatement(inputs):
    """torch Conv1d under torch's own norms in float64 == spectral64 / weight_norm64 + forward64, buffers included, in both modes"""
    state, y, y_hat = inputs
    for training in (False, True):
        twin = DH.TwinMSD().double()
        twin.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
        twin.train(training)
        rs, gs, frs, fgs = twin(y.double(), y_hat.double())
        fw = DH.msd_forward64(state, y, y_hat, training)
        for i in range(3):
            for l in range(DH.N):
                for got, want in ((frs[i][l], fw['r'][i]['fmap'][l]), (fgs[i][l], fw['g'][i]['fmap'][l])):
                    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        sd = twin.state_dict()
        for p in DH.prefixes(0):
            for n in ('weight_u', 'weight_v'):
                assert float((sd[p + n] - fw['state'][p + n]).abs().max()) <= 1e-12
                if 'conv_post' not in p:                        # a one-row matrix: the start is already the fixed point of the iteration
                    assert torch.equal(sd[p + n], state[p + n].double()) == (not training)
        fl, gen, rl, gl = DH.twin_losses((rs, gs, frs, fgs))
        for got, want in zip((fl, gen, rl, gl), DH.msd_losses64(fw)):
            assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


# The chained RULE bounds below are worst cases that grow by a large factor per layer: past the first layers they hold whatever the restatement
# computes.  What decides is the observed error: a float32 run of this network agrees with float64 to about 1e-6 of a tensor's largest value,
# so every tensor must lie within CLOSE of its float64 restatement's largest absolute value, every loss within CLOSE_LOSS relative, the unit
# vectors of the power iteration within CLOSE_UNIT - one to two orders above float32 noise, orders below any wrong term.
CLOSE, CLOSE_LOSS, CLOSE_UNIT = 1e-4, 1e-5, 1e-5


def close(name, got, want, scale):
    err = float((got - want).abs().max())
    assert err <= CLOSE * float(scale.abs().max()), f'{name}: max error {err:.3e} against the largest value {float(scale.abs().max()):.3e}'


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_restatement_reproduces_the_reference_forward(fx, restated, mode):
    fw, _ = restated[mode]
    worst = 0.0
    for i in range(3):
        for s, side in (('r', 'fr'), ('g', 'fg')):
            f = fw[s][i]
            out, e_out = f['fmap'][DH.N - 1].reshape(1, -1), f['e_fmap'][DH.N - 1].reshape(1, -1)
            err = (torch.from_numpy(fx[f'{mode}/{s}{i}']).double() - out).abs()
            assert bool((err <= e_out).all()), (mode, s, i, float((err / e_out).max()))
            close(f'{mode} y_d_{s}s[{i}]', torch.from_numpy(fx[f'{mode}/{s}{i}']).double(), out, out)
            for l in range(DH.N):
                idx = torch.from_numpy(fx[f'idx/{side}{i}_{l}'].astype(np.int64))
                want, e = f['fmap'][l].reshape(-1)[idx], f['e_fmap'][l].reshape(-1)[idx]
                err = (torch.from_numpy(fx[f'{mode}/{side}{i}_{l}']).double() - want).abs()
                assert bool((err <= e).all()), (mode, side, i, l, float((err / e).max()))
                close(f'{mode} {side}{i}_{l}', torch.from_numpy(fx[f'{mode}/{side}{i}_{l}']).double(), want, f['fmap'][l])
                worst = max(worst, float((err / e).max()))
    assert worst > 0.0                                          # the comparison is not vacuous: float32 and float64 do differ
    losses = DH.msd_losses64(fw)
    for got, want, e in zip(fx[f'{mode}/losses'], losses, DH.msd_loss_bounds(fw)):
        assert abs(got - float(want)) <= e + 64 * DH.U * abs(float(want))              # the reference sums the means in float32
        assert abs(got - float(want)) <= CLOSE_LOSS * abs(float(want)), (mode, got, float(want))


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_restatement_reproduces_the_reference_gradients_and_buffers(fx, restated, inputs, mode):
    fw, bw = restated[mode]
    d, e = bw['dy_hat']
    err = (torch.from_numpy(fx[f'{mode}/dy_hat']).double() - d).abs()
    assert bool((err <= e).all()), float((err / e).max())
    close(f'{mode} dy_hat', torch.from_numpy(fx[f'{mode}/dy_hat']).double(), d, d)
    keys = sorted(k[len('eval/grad/'):] for k in fx if k.startswith('eval/grad/'))
    assert keys == sorted(bw['grads'])
    for k in keys:
        v, e = bw['grads'][k]
        idx = torch.from_numpy(fx[f'idx/grad/{k}'].astype(np.int64))
        err = (torch.from_numpy(fx[f'{mode}/grad/{k}']).double() - v.reshape(-1)[idx]).abs()
        assert bool((err <= e.reshape(-1)[idx]).all()), (mode, k, float((err / e.reshape(-1)[idx]).max()))
        close(f'{mode} grad {k}', torch.from_numpy(fx[f'{mode}/grad/{k}']).double(), v.reshape(-1)[idx], v)
    for l, p in enumerate(DH.prefixes(0)):
        got = torch.from_numpy(fx[f'{mode}/u{l}']).double()
        if mode == 'eval':
            assert torch.equal(got, inputs[0][p + 'weight_u'].double())
        else:
            sp = fw['g'][0]['w']['sp'][l]                       # the second call's buffers
            assert bool(((got - sp['u']).abs() <= sp['e_u'] + DH.U).all()), l
            assert float((got - sp['u']).abs().max()) <= CLOSE_UNIT, l
            assert got.numel() == 1 or not torch.equal(got, inputs[0][p + 'weight_u'].double())


def test_helper_backward_is_the_autograd_of_its_forward():
    gen = torch.Generator().manual_seed(5)
    ws, bs = DH.synth_plain(11)
    ws = [w.double().requires_grad_(True) for w in ws]
    bs = [b.double().requires_grad_(True) for b in bs]
    x = torch.randn(2, 1, 77, generator=gen, dtype=torch.float64, requires_grad=True)
    f = DH.forward64(x, ws, bs)
    cts = [torch.randn(a.shape, generator=gen, dtype=torch.float64) for a in f['fmap']]
    g_out = torch.randn(2, f['fmap'][7].shape[2], generator=gen, dtype=torch.float64)
    loss = sum((a * c).sum() for a, c in zip(f['fmap'], cts)) + (f['fmap'][7].reshape(2, -1) * g_out).sum()
    loss.backward()
    bw = DH.backward64(g_out, cts, x.detach(), [w.detach() for w in ws], [a.detach() for a in f['fmap']])
    for l in range(DH.N):
        assert float((bw['dw'][l][0] - ws[l].grad).abs().max()) <= 1e-10 * max(1.0, float(ws[l].grad.abs().max()))
        assert float((bw['db'][l][0] - bs[l].grad).abs().max()) <= 1e-10 * max(1.0, float(bs[l].grad.abs().max()))
    assert float((bw['dx'][0] - x.grad).abs().max()) <= 1e-10 * max(1.0, float(x.grad.abs().max()))
    g = torch.randn(2, 1, 38, generator=gen, dtype=torch.float64)
    assert DH.pool_backward64(g, 77).shape == (2, 1, 77)
    assert abs(float((DH.pool_backward64(g, 77) * x.detach()).sum() - (g * DH.pool64(x.detach())).sum())) <= 1e-10


def test_hgd_symbols_declared_bound_and_exported():
    from tests.test_abi import _header_symbols
    names = [n for n in _header_symbols('dsv.h', 'dsv_') if n.startswith('dsv_hgd_')]
    assert names == ['dsv_hgd_avgpool', 'dsv_hgd_avgpool_backward', 'dsv_hgd_pool_samples']
    lib = _lib.load()
    for n in names:
        assert n in _lib.SYMBOLS_VOC and hasattr(lib, n), n
    assert [lib.dsv_hgd_pool_samples(t) for t in (1, 2, 3, 4, 5, 1061)] == [-1, 1, 1, 2, 2, 530]
    # refused before any launch
    assert lib.dsv_hgd_avgpool(4096, 8192, 1, 1, 1, None) == -1 and b'bad shape' in lib.dsd_last_error()
    assert lib.dsv_hgd_avgpool(4096, 8192, 1, 8, 7, None) == -1 and b'row stride' in lib.dsd_last_error()
    assert lib.dsv_hgd_avgpool_backward(4096, 4096 + 8, 1, 8, 4, None) == -1 and b'overlap' in lib.dsd_last_error()      # partly overlapping
    assert lib.dsv_hgd_avgpool(4096, 4096, 1, 8, 8, None) == -1 and b'overlap' in lib.dsd_last_error()
