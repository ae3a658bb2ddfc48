"""CPU: the test infrastructure of the HiFi-GAN period discriminator - the fixture recorded from the reference (tests/golden/hifigan_mpd_ref.npz), its
keys and shapes, the float64 restatement of tests/hifigan_mpd_helpers.py against the recorded reference numbers - and the host side of what
diffsinger_amd/hifigan_disc.py adds for it (shapes, refusals, the C ABI's checks; the kernels are checked in tests/test_gpu_hifigan_mpd.py)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from diffsinger_amd import _lib
from tests import hifigan_mpd_helpers as MH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the figures tests/test_hifigan_disc_host.py uses: every tensor within CLOSE of its largest value, every loss within CLOSE_LOSS relative
CLOSE, CLOSE_LOSS = 1e-4, 1e-5


@pytest.fixture(scope='module')
def fx():
    return MH.fixture()


@pytest.fixture(scope='module')
def inputs():
    return MH.fixture_inputs()


@pytest.fixture(scope='module')
def restated(inputs):
    """the float64 restatement, computed once: (forward, backward)"""
    state, y, y_hat = inputs
    fw = MH.mpd_forward64(state, y, y_hat)
    return fw, MH.mpd_backward64(fw, state, MH.FIXTURE_T)


def close(name, got, want, scale=None):
    scale = want if scale is None else scale
    err, big = float((got - want).abs().max()), float(scale.abs().max())
    print(f'{name}: max error {err:.3e}, largest value {big:.3e}')
    assert err <= CLOSE * big, f'{name}: max error {err:.3e} against the largest value {big:.3e}'


def test_fixture_is_small_and_complete(fx):
    assert os.path.getsize(MH.FIXTURE) <= 600 * 1000
    meta = fx['meta']
    assert (meta['B'], meta['T'], meta['seed'], meta['samples']) == (MH.FIXTURE_B, MH.FIXTURE_T, MH.FIXTURE_SEED, MH.FIXTURE_SAMPLES)
    assert len(meta['keys']) == 90 and len(meta['shapes']) == 90
    assert fx['losses'].shape == (4,) and fx['dy_hat'].shape == (1, 1, 300)
    for i, p in enumerate(MH.PERIODS):
        hs = MH.heights(300, p)
        assert fx[f'r{i}'].shape == (1, hs[6] * p) == fx[f'g{i}'].shape
        for l in range(MH.N):
            n = min(MH.FIXTURE_SAMPLES, MH.LAYERS[l][1] * hs[l + 1] * p)
            assert fx[f'fr{i}_{l}'].shape == (n,) == fx[f'idx/fg{i}_{l}'].shape
    grads = [k for k in fx if k.startswith('grad/')]
    assert len(grads) == 90 and all(fx[k].size <= MH.FIXTURE_SAMPLES for k in grads)
    assert not [k for k in fx if k.startswith('state')]         # 41 M parameters: none stored


def test_keys_and_shapes_are_the_references(fx, inputs):
    """the twin module, the restated shapes and the product's module carry the reference's 90 state-dict entries; a strict load succeeds"""
    from diffsinger_amd import MultiPeriodDiscriminator
    for mod in (MH.TwinMPD(), MultiPeriodDiscriminator()):
        sd = mod.state_dict()
        assert sorted(sd) == sorted(fx['meta']['keys'])
        assert {k: list(v.shape) for k, v in sd.items()} == dict(zip(fx['meta']['keys'], fx['meta']['shapes']))
        assert {k: tuple(v.shape) for k, v in sd.items()} == MH.module_shapes()
        mod.load_state_dict(inputs[0], strict=True)
    assert list(MH.TwinMPD().state_dict()) == fx['meta']['keys']
    assert sum(v.numel() for v in inputs[0].values()) == 5 * (8215712 + 2 * 2721)    # 41.1 M: weight_v, weight_g, bias
    m = MultiPeriodDiscriminator()
    m.load_state_dict(inputs[0], strict=True)
    m.remove_weight_norm()
    assert sorted(m.state_dict()) == sorted({k.replace('weight_v', 'weight') for k in fx['meta']['keys'] if not k.endswith('weight_g')})
    m2 = MultiPeriodDiscriminator()
    m2.load_state_dict(m.state_dict(), strict=True)            # a state saved after remove_weight_norm() loads into a fresh module


def test_heights_are_conv2d_s():
    from diffsinger_amd.hifigan_disc import period_heights
    lib = _lib.load()
    for p in MH.PERIODS:
        for T in (p, p + 1, 292, 300):
            x = torch.zeros(1, 1, T)
            h = MH.fold64(x, p)
            got = [h.shape[2]]
            for l, (ci, co, k, s) in enumerate(MH.LAYERS):
                h = F.conv2d(h.expand(1, ci, -1, -1), torch.zeros(1, ci, k, 1), None, stride=(s, 1), padding=((k - 1) // 2, 0))
                got.append(h.shape[2])
                assert h.shape[3] == p
            assert MH.heights(T, p) == got, (p, T)
            assert period_heights(T, p) == got[:6], (p, T)
            assert lib.dsv_hgp_folded_samples(T, p) == got[0] * p
            assert [lib.dsv_hgp_height(a, 3) for a in got[:4]] == got[1:5] and lib.dsv_hgp_height(got[4], 1) == got[5]
    # the table of the GPU tests
    assert MH.heights(2, 2)[:5] == [1, 1, 1, 1, 1] and MH.heights(12, 11)[:5] == [2, 1, 1, 1, 1]
    assert MH.heights(292, 3)[:5] == [98, 33, 11, 4, 2] and MH.heights(300, 3)[:5] == [100, 34, 12, 4, 2]
    assert MH.heights(1454, 5)[:5] == [291, 97, 33, 11, 4] and MH.heights(2121, 2)[:5] == [1061, 354, 118, 40, 14]
    assert MH.heights(300, 7)[:5] == [43, 15, 5, 2, 1] and MH.heights(300, 11)[:5] == [28, 10, 4, 2, 1]


def test_conv2d_on_the_folded_view_is_conv1d_on_the_rows():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 47, generator=gen, dtype=torch.float64)
    w = torch.randn(4, 1, 5, 1, generator=gen, dtype=torch.float64)
    for p in (3, 5):
        xf = MH.fold64(x, p)
        a = F.conv2d(xf, w, None, stride=(3, 1), padding=(2, 0))
        rows = xf.permute(0, 3, 1, 2).reshape(2 * p, 1, -1)
        b = F.conv1d(rows, w[:, :, :, 0], None, stride=3, padding=2).reshape(2, p, 4, -1).permute(0, 2, 3, 1)
        assert torch.equal(a, b)
        g = torch.randn(xf.shape, generator=gen, dtype=torch.float64)
        dx = MH.fold_backward64(g, 47, p).reshape(2, 47)
        gf = g.reshape(2, -1)
        want = gf[:, :47].clone()
        for i in range(47, gf.shape[1]):
            want[:, 2 * 46 - i] += gf[:, i]
        assert torch.equal(dx, want)


def test_restatement_reproduces_the_reference(fx, restated):
    fw, bw = restated
    for i in range(len(MH.PERIODS)):
        for s in ('r', 'g'):
            close(f'{s}{i}', fw[s][i]['fmap'][MH.N - 1].reshape(1, -1), torch.from_numpy(fx[f'{s}{i}']).double())
            for l in range(MH.N):
                full = fw[s][i]['fmap'][l].reshape(-1)
                close(f'f{s}{i}_{l}', full[torch.from_numpy(fx[f'idx/f{s}{i}_{l}']).long()], torch.from_numpy(fx[f'f{s}{i}_{l}']).double(), full)
    for name, got, want in zip(('feature', 'generator', 'r', 'g'), MH.mpd_losses64(fw), fx['losses']):
        rel = abs(float(got) - float(want)) / abs(float(want))
        print(f'{name}_loss: relative error {rel:.3e}')
        assert rel <= CLOSE_LOSS, (name, float(got), float(want))
    close('dy_hat', bw['dy_hat'][0], torch.from_numpy(fx['dy_hat']).double())
    assert len(bw['grads']) == 90
    for k, (v, _) in bw['grads'].items():
        close('grad/' + k, v.reshape(-1)[torch.from_numpy(fx['idx/grad/' + k]).long()], torch.from_numpy(fx['grad/' + k]).double(), v)


def test_twin_module_is_the_functional_restatement(inputs, restated):
    state, y, y_hat = inputs
    twin = MH.TwinMPD().double()
    twin.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
    rs, gs, frs, fgs = twin(y.double(), y_hat.double())
    fw = restated[0]
    for i in range(len(MH.PERIODS)):
        for l in range(MH.N):
            for got, want in ((frs[i][l], fw['r'][i]['fmap'][l]), (fgs[i][l], fw['g'][i]['fmap'][l])):
                assert got.shape == want.shape
                assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for got, want in zip(MH.twin_losses((rs, gs, frs, fgs)), MH.mpd_losses64(fw)):
        assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


def test_fixture_seed_keeps_kinks_and_ties_apart(inputs, restated):
    """the float32 CPU twin flips no LeakyReLU mask and no L1 sign against float64 on the fixture's inputs, and the margin the seed was chosen
    for is what hifigan_mpd_helpers says"""
    state, y, y_hat = inputs
    twin = MH.TwinMPD()
    twin.load_state_dict(state, strict=True)
    with torch.no_grad():
        _, _, frs32, fgs32 = twin(y, y_hat)
    frs, fgs = [f['fmap'] for f in restated[0]['r']], [f['fmap'] for f in restated[0]['g']]
    for i in range(len(MH.PERIODS)):
        for l in range(MH.N):
            assert torch.equal(frs32[i][l] > 0, frs[i][l] > 0) and torch.equal(fgs32[i][l] > 0, fgs[i][l] > 0), (i, l)
            assert torch.equal(torch.sign(frs32[i][l] - fgs32[i][l]).double(), torch.sign(frs[i][l] - fgs[i][l])), (i, l)
    margin = MH.kink_and_tie_margin(frs, fgs, frs32, fgs32)
    print(f'smallest |pre-activation| or |r - g| in units of the float32 deviation of its map: {margin:.3f}')
    assert margin >= 0.5


def test_activations_stay_order_one(restated):
    """the seeded state keeps every feature map of the fixture's shape at O(1): nothing vanishes or blows up with depth"""
    for i in range(len(MH.PERIODS)):
        for l in range(MH.N - 1):
            rms = float(restated[0]['g'][i]['fmap'][l].pow(2).mean().sqrt())
            assert 0.05 < rms < 20.0, (i, l, rms)


def test_inputs_are_validated_before_device_work():
    import diffsinger_amd
    from diffsinger_amd import hifigan_disc as HD
    for name in ('disc_p_op', 'feature_loss', 'DiscriminatorP', 'MultiPeriodDiscriminator', 'hifigan_adversarial_losses',
                 'hifigan_discriminator_losses'):
        assert getattr(diffsinger_amd, name) is getattr(HD, name)
    n0 = HD.launch_count()
    for kw, what in ((dict(use_cond=True), 'use_cond'), (dict(c_in=2), 'c_in'), (dict(use_spectral_norm=True), 'spectral norm'),
                     (dict(kernel_size=3), 'kernel_size'), (dict(stride=2), 'stride')):
        with pytest.raises(NotImplementedError, match=what):
            HD.DiscriminatorP(3, **kw)
    with pytest.raises(NotImplementedError, match='use_cond'):
        HD.MultiPeriodDiscriminator(use_cond=True)
    with pytest.raises(NotImplementedError, match='c_in'):
        HD.MultiPeriodDiscriminator(c_in=2)
    d = HD.DiscriminatorP(11)
    ws, bs = MH.synth_plain(1)
    for T in (1, 5):                                             # a reflect pad of 10 and 6 samples: F.pad refuses both
        with pytest.raises(ValueError, match='reflect pad'):
            d(torch.zeros(1, 1, T))
        with pytest.raises(ValueError, match='reflect pad'):
            HD.disc_p_op(torch.zeros(1, 1, T), 11, ws, bs)
        with pytest.raises(RuntimeError):
            F.pad(torch.zeros(1, 1, T), (0, 11 - T), 'reflect')
    assert HD.period_heights(6, 11) == [1, 1, 1, 1, 1, 1] and HD.period_heights(11, 11)[0] == 1
    with pytest.raises(ValueError, match='no CPU path'):
        d(torch.zeros(1, 1, 300))
    with pytest.raises(ValueError, match=r'\[B\]\[1\]\[T\]'):
        d(torch.zeros(1, 2, 300))
    with pytest.raises(ValueError, match='float32'):
        d(torch.zeros(1, 1, 300, dtype=torch.float64))
    with pytest.raises(ValueError, match='period'):
        HD.disc_p_op(torch.zeros(1, 1, 300), 0, ws, bs)
    with pytest.raises(NotImplementedError, match='mel'):
        d(torch.zeros(1, 1, 300), torch.zeros(1, 80, 2))
    with pytest.raises(ValueError, match='no CPU path'):
        HD.MultiPeriodDiscriminator()(torch.zeros(1, 1, 300), torch.zeros(1, 1, 300))
    with pytest.raises(ValueError, match='no CPU path'):
        HD.feature_loss([[torch.zeros(3)]], [[torch.zeros(3)]])
    with pytest.raises(ValueError, match='as many'):
        HD.feature_loss([[torch.zeros(3)]], [[]])
    assert HD.launch_count() == n0


def _header_symbols(prefix):
    src = open(os.path.join(ROOT, 'include', 'dsv.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(' + prefix + r'[a-z0-9_]+)\s*\(', src)))


def test_abi_is_declared_bound_and_refuses_bad_arguments_on_the_host():
    from diffsinger_amd import build
    names = _header_symbols('dsv_hgp_')
    assert len(names) == 20
    lib = _lib.load()
    for n in names:
        assert n in _lib.SYMBOLS_VOC and hasattr(lib, n), n
    for f in ('hifigan_mpd.hpp', 'hifigan_mpd_abi.hpp'):
        assert os.path.join(ROOT, 'diffsinger_amd', 'csrc', f) in build.DEPS
    err = lambda: lib.dsd_last_error()
    assert [lib.dsv_hgp_folded_samples(t, p) for t, p in ((2, 2), (12, 11), (6, 11), (5, 11), (300, 7), (1, 1), (1, 2), (8, 65))] == [2, 22, 11, -1, 301, 1, -1, -1]
    assert [lib.dsv_hgp_dgrad_phase_taps(3, r) for r in range(3)] == [0b00100, 0b01001, 0b10010] and lib.dsv_hgp_dgrad_phase_taps(1, 0) == 0b11111
    assert lib.dsv_hgp_dgrad_phase_taps(2, 0) == -1 and lib.dsv_hgp_dgrad_phase_taps(3, 3) == -1
    pf = lib.dsv_packed_floats
    assert lib.dsv_hgp_dgrad_packed_offset(32, 128, 3, 3) == pf(32, 128, 1) + 2 * pf(32, 128, 2)
    assert lib.dsv_hgp_dgrad_packed_offset(32, 128, 3, 1) == pf(32, 128, 1) and lib.dsv_hgp_dgrad_packed_offset(1024, 1024, 1, 1) == pf(1024, 1024, 5)
    # the weight gradient splits its positions where the output tiles alone do not fill the chip: the training shape (2 B = 32, T = 8192, period 2)
    assert lib.dsv_hgp_wgrad_splits(32, 32, 128, 456, 2) == 57 and lib.dsv_hgp_wgrad_splits(32, 128, 512, 152, 2) == 19
    assert lib.dsv_hgp_wgrad_splits(32, 512, 1024, 51, 2) == 7 and lib.dsv_hgp_wgrad_splits(32, 1024, 1024, 51, 2) == 1
    assert lib.dsv_hgp_wgrad_workspace_floats(32, 1024, 1024, 51, 2) == 0
    assert lib.dsv_hgp_wgrad_workspace_floats(32, 32, 128, 456, 2) == 57 * 32 * 128 * 5
    assert lib.dsv_hgp_wgrad_splits(1, 32, 128, 4, 2) == 1 and lib.dsv_hgp_wgrad_splits(1, 30, 128, 4, 2) == -1
    assert lib.dsv_hgp_edge_workspace_floats(2, 100, 3, 32, 5) == 32 * 6 and lib.dsv_hgp_edge_workspace_floats(2, 100, 3, 32, 6) == -1
    assert lib.dsv_hgp_l1_blocks(1) == 1 and lib.dsv_hgp_l1_blocks(1 << 30) == 256 and lib.dsv_hgp_l1_blocks(0) == -1
    a, b = 1 << 20, 1 << 24                                       # addresses never dereferenced: every refusal precedes the first launch
    assert lib.dsv_hgp_fold(None, b, 1, 8, 8, 2, None) == -1 and b'null' in err()
    assert lib.dsv_hgp_fold(a, b, 1, 5, 5, 11, None) == -1 and b'reflect pad' in err()
    assert lib.dsv_hgp_fold(a, b, 1, 8, 7, 2, None) == -1 and b'row stride' in err()
    assert lib.dsv_hgp_fold(a, a + 16, 1, 8, 8, 2, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_fold(a, b, 40000, 8, 8, 2, None) == -1 and b'B * period <= 65535' in err()
    assert lib.dsv_hgp_fold_backward(a, a, 1, 8, 2, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_first(a, a, None, b, 1, 32, 0, 2, 3, 0.1, None) == -1 and b'bad shape' in err()
    assert lib.dsv_hgp_first(a, a, None, b, 1, 32, 4, 2, 2, 0.1, None) == -1 and b'stride' in err()
    assert lib.dsv_hgp_first(a, a, None, b, 1, 32, 4, 2, 3, 1.5, None) == -1 and b'negative_slope' in err()
    assert lib.dsv_hgp_conv(a, a, None, b, 1, 48, 128, 4, 2, 3, 0.1, None) == -1 and b'multiples of 32' in err()
    assert lib.dsv_hgp_conv(a, a, None, a + 64, 1, 32, 128, 4, 2, 3, 0.1, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_conv(a, a, None, b, 32768, 32, 128, 4, 2, 3, 0.1, None) == -1 and b'B * period <= 65535' in err()
    assert lib.dsv_hgp_conv_dgrad(a, a, None, None, a, 1, 32, 128, 4, 2, 3, 0.1, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_conv_dgrad(a, None, None, None, b, 1, 32, 128, 4, 2, 3, 0.1, None) == -1 and b'null' in err()
    assert lib.dsv_hgp_conv_wgrad(a, a, None, b, None, 4, 32, 128, 400, 2, 3, None) == -1 and b'need the workspace' in err()
    assert lib.dsv_hgp_conv_wgrad(a, a, None, b, None, 4, 32, 128, 400, 65, 3, None) == -1 and b'period' in err()
    assert lib.dsv_hgp_post(a, a, None, a + 8, 1, 1024, 4, 2, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_post_backward(a, None, b, a, None, a, a, None, b, 1, 1024, 4, 2, 0.1, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_post_backward(a, None, b, a, None, a, a, None, b + (1 << 20), 1, 1024, 4, 2, 0.0, None) == -1 and b'negative_slope' in err()
    assert lib.dsv_hgp_l1_partial(a, a, a + 4, 8, None) == -1 and b'aligned to 8 bytes' in err()
    assert lib.dsv_hgp_l1_partial(a, a, b, 0, None) == -1 and b'bad shape' in err()
    assert lib.dsv_hgp_l1_final(b, 0, a, None) == -1 and b'nblocks' in err()
    assert lib.dsv_hgp_l1_backward(a, a, a, None, b, 8, None) == -1 and b'null' in err()
