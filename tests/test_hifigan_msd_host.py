"""CPU: the host side of the HiFi-GAN scale discriminator's stack (include/dsv.h section "HiFi-GAN scale discriminator stack",
csrc/hifigan_msd_abi.hpp) and of what diffsinger_amd/hifigan_disc.py adds for it - names, sizes, refusals before any launch, the modules' state
dict against the fixture recorded from the reference.  The kernels are checked in tests/test_gpu_hifigan_msd.py."""
import os
import re

import pytest
import torch

from diffsinger_amd import _lib
from tests import hifigan_disc_helpers as DH
from tests import hifigan_msd_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED = [(ci, co, s, g) for ci, co, k, s, g in DH.LAYERS[1:6]]


def _header_symbols(prefix):
    src = open(os.path.join(ROOT, 'include', 'dsv.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(' + prefix + r'[a-z0-9_]+)\s*\(', src)))


def test_abi_is_declared_bound_and_exported():
    from diffsinger_amd import build
    names = _header_symbols('dsv_hgs_')
    assert names == sorted(['dsv_hgs_out_len', 'dsv_hgs_first_workspace_floats', 'dsv_hgs_first', 'dsv_hgs_first_backward', 'dsv_hgs_packed_floats',
                            'dsv_hgs_pack', 'dsv_hgs_gconv', 'dsv_hgs_gconv_dgrad', 'dsv_hgs_wgrad_splits', 'dsv_hgs_wgrad_workspace_floats',
                            'dsv_hgs_gconv_wgrad'])
    lib = _lib.load()
    for n in names:
        assert n in _lib.SYMBOLS_VOC and hasattr(lib, n), n
    for f in ('hifigan_msd.hpp', 'hifigan_msd_abi.hpp'):
        assert os.path.join(ROOT, 'diffsinger_amd', 'csrc', f) in build.DEPS
    # the period discriminator's and the pooling's names are as they were
    assert len(_header_symbols('dsv_hgp_')) == 20 and len(_header_symbols('dsv_hgd_')) == 3


def test_size_functions():
    from diffsinger_amd.hifigan_disc import scale_lengths
    lib = _lib.load()
    for T in (1, 41, 280, 300, 513, 1024, 1030, 2121, 8192):
        want = DH.lengths(T)
        assert scale_lengths(T) == want
        L, got = T, []
        for ci, co, k, s, g in DH.LAYERS[1:6]:
            L = lib.dsv_hgs_out_len(L, s)
            got.append(L)
        assert got == want[1:6], T
    assert lib.dsv_hgs_out_len(0, 2) == -1 and lib.dsv_hgs_out_len(8, 3) == -1
    # the table of the GPU tests
    assert DH.lengths(1)[:6] == [1] * 6 and DH.lengths(41)[:5] == [41, 21, 11, 3, 1]
    assert DH.lengths(280)[2:5] == [70, 18, 5] and DH.lengths(300)[2:5] == [75, 19, 5]
    assert DH.lengths(513)[:5] == [513, 257, 129, 33, 9] and DH.lengths(1030)[:5] == [1030, 515, 258, 65, 17]
    assert DH.lengths(2121)[:5] == [2121, 1061, 531, 133, 34]
    for ci, co, s, g in GROUPED:
        n = co * (ci // g) * 41
        assert lib.dsv_hgs_packed_floats(ci, co, s, g, 0) == n               # forward: the weights, reordered
        rows = max(ci // g, 16)                                              # data gradient: ci_g rows per group (8 sit in a 16-row block), all 41 taps over the phases
        assert lib.dsv_hgs_packed_floats(ci, co, s, g, 1) == g * rows * (co // g) * 41
    assert lib.dsv_hgs_packed_floats(128, 128, 2, 16, 0) == -1 and lib.dsv_hgs_packed_floats(128, 128, 2, 4, 2) == -1
    assert lib.dsv_hgs_packed_floats(32, 128, 3, 1, 0) == -1
    # first layer: splits of 4096 positions, 15 taps + the bias per channel
    assert lib.dsv_hgs_first_workspace_floats(1, 1, 128) == 128 * 16 and lib.dsv_hgs_first_workspace_floats(3, 2121, 128) == 2 * 128 * 16
    assert lib.dsv_hgs_first_workspace_floats(0, 5, 128) == -1 and lib.dsv_hgs_first_workspace_floats(1, 5, 0) == -1
    # weight gradient: units of 32 positions per batch row, 16 units per split, doubled while the launch would exceed 1024 workgroups
    assert lib.dsv_hgs_wgrad_splits(3, 128, 128, 1061, 2, 4) == 7 and lib.dsv_hgs_wgrad_workspace_floats(3, 128, 128, 1061, 2, 4) == 7 * 128 * 32 * 41
    assert lib.dsv_hgs_wgrad_splits(1, 128, 128, 21, 2, 4) == 1 and lib.dsv_hgs_wgrad_workspace_floats(1, 128, 128, 21, 2, 4) == 0
    assert lib.dsv_hgs_wgrad_splits(3, 1024, 1024, 34, 1, 16) == 1
    # the training shape, 32 rows of 8192 samples: 16 output tiles x 64 splits, 128 x 8
    assert lib.dsv_hgs_wgrad_splits(32, 128, 128, 4096, 2, 4) == 64 and lib.dsv_hgs_wgrad_splits(32, 1024, 1024, 128, 1, 16) == 8
    assert lib.dsv_hgs_wgrad_splits(32, 128, 128, 4096, 2, 16) == -1 and lib.dsv_hgs_wgrad_splits(0, 128, 128, 4096, 2, 4) == -1


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.dsd_last_error()
    a, b = 1 << 20, 1 << 28                                       # addresses never dereferenced: every refusal precedes the first launch
    assert lib.dsv_hgs_first(None, a, None, b, 1, 128, 8, 8, 0.1, None) == -1 and b'null' in err()
    assert lib.dsv_hgs_first(a, a, None, b, 1, 128, 0, 8, 0.1, None) == -1 and b'bad shape' in err()
    assert lib.dsv_hgs_first(a, a, None, b, 1, 128, 8, 7, 0.1, None) == -1 and b'row stride' in err()
    assert lib.dsv_hgs_first(a, a, None, b, 1, 128, 8, 8, 1.0, None) == -1 and b'negative_slope' in err()
    assert lib.dsv_hgs_first(a, a, None, a + 16, 1, 128, 8, 8, 0.1, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgs_first(a, a, None, b, 70000, 128, 8, 8, 0.1, None) == -1 and b'bad shape' in err()
    assert lib.dsv_hgs_first_backward(a, a, a, None, b, None, None, 1, 128, 8, 8, None) == -1 and b'null' in err()
    assert lib.dsv_hgs_first_backward(a, a, a, b, b, None, a + 64, 1, 128, 8, 8, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgs_first_backward(a, a, a, b, b, None, None, 1, 128, 8, 4, None) == -1 and b'row stride' in err()
    assert lib.dsv_hgs_pack(a, None, 128, 128, 2, 4, 0, None) == -1 and b'null' in err()
    assert lib.dsv_hgs_pack(a, b, 128, 128, 2, 8, 0, None) == -1 and b'none of the grouped layers' in err()
    assert lib.dsv_hgs_pack(a, b, 128, 128, 2, 4, 2, None) == -1 and b'dgrad' in err()
    assert lib.dsv_hgs_pack(a, b + 4, 128, 128, 2, 4, 0, None) == -1 and b'aligned to 16 bytes' in err()
    assert lib.dsv_hgs_pack(a, a + 1024, 128, 128, 2, 4, 0, None) == -1 and b'overlap' in err()
    for name in ('dsv_hgs_gconv', 'dsv_hgs_gconv_dgrad'):
        f = getattr(lib, name)
        extra = (None,) if name.endswith('dgrad') else ()
        assert f(a, None, None, *extra, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'null' in err()
        for geo in ((128, 128, 2, 16), (128, 128, 4, 4), (64, 128, 2, 4), (1024, 1024, 1, 1), (1, 128, 1, 1)):
            assert f(a, a, None, *extra, b, 1, geo[0], geo[1], 64, geo[2], geo[3], 0.1, None) == -1 and b'none of the grouped layers' in err(), geo
        assert f(a, a, None, *extra, b, 1, 128, 128, 0, 2, 4, 0.1, None) == -1 and b'bad shape' in err()
        assert f(a, a, None, *extra, b, 65536, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'bad shape' in err()
        assert f(a, a, None, *extra, b, 1, 128, 128, 64, 2, 4, 0.0, None) == -1 and b'negative_slope' in err()
        assert f(a, a + 4, None, *extra, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'aligned to 16 bytes' in err()
        assert f(a, a, None, *extra, a + 256, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'overlap' in err()
    # every operand a call reads against every range it writes
    c = 1 << 30
    assert lib.dsv_hgs_first(a, b, None, b, 1, 128, 8, 8, 0.1, None) == -1 and b'overlap' in err()                        # w in out
    assert lib.dsv_hgs_first(a, a, b + 64, b, 1, 128, 8, 8, 0.1, None) == -1 and b'overlap' in err()                   # bias in out
    assert lib.dsv_hgs_first_backward(a, a, a, b, b, None, None, 1, 128, 8, 8, None) == -1 and b'overlap' in err()      # workspace on dw
    assert lib.dsv_hgs_first_backward(a, c, a, b, c, None, None, 1, 128, 8, 8, None) == -1 and b'overlap' in err()      # x on dw
    assert lib.dsv_hgs_first_backward(a, a, a, b, c, c + 4 * 100, None, 1, 128, 8, 8, None) == -1 and b'overlap' in err()       # db in dw
    assert lib.dsv_hgs_gconv(a, b, None, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'overlap' in err()               # w_packed on out
    assert lib.dsv_hgs_gconv(a, a, b + 4, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'overlap' in err()              # bias in out
    assert lib.dsv_hgs_gconv_dgrad(a, a, b, None, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'overlap' in err()      # cot on out
    assert lib.dsv_hgs_gconv_dgrad(a, a, None, b + 64, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'overlap' in err() # saved in out
    assert lib.dsv_hgs_gconv_dgrad(a, b, None, None, b, 1, 128, 128, 64, 2, 4, 0.1, None) == -1 and b'overlap' in err()   # w_packed on out
    assert lib.dsv_hgs_gconv_wgrad(a, a, None, b, b + 4, 1, 128, 128, 64, 2, 4, None) == -1 and b'overlap' in err()      # db in dw
    assert lib.dsv_hgs_gconv_wgrad(a, a, b, b, None, 3, 128, 128, 2121, 2, 4, None) == -1 and b'overlap' in err()         # workspace on dw
    assert lib.dsv_hgs_gconv_wgrad(a, None, None, b, None, 1, 128, 128, 64, 2, 4, None) == -1 and b'null' in err()
    assert lib.dsv_hgs_gconv_wgrad(a, a, None, b, None, 1, 128, 256, 64, 2, 4, None) == -1 and b'none of the grouped layers' in err()
    assert lib.dsv_hgs_gconv_wgrad(a, a, None, b, None, 3, 128, 128, 2121, 2, 4, None) == -1 and b'need the workspace' in err()
    assert lib.dsv_hgs_gconv_wgrad(a, a, None, a + 64, None, 1, 128, 128, 64, 2, 4, None) == -1 and b'overlap' in err()
    assert lib.dsv_hgs_gconv_wgrad(a, a, None, b, None, 1, 128, 128, 0, 2, 4, None) == -1 and b'bad shape' in err()


def test_inputs_are_validated_before_device_work():
    import diffsinger_amd
    from diffsinger_amd import hifigan_disc as HD
    for name in ('disc_s_op', 'DiscriminatorS', 'MultiScaleDiscriminator'):
        assert getattr(diffsinger_amd, name) is getattr(HD, name) and name in diffsinger_amd.__all__
    n0 = HD.launch_count()
    for kw, what in ((dict(use_cond=True), 'use_cond'), (dict(c_in=2), 'c_in')):
        with pytest.raises(NotImplementedError, match=what):
            HD.DiscriminatorS(**kw)
        with pytest.raises(NotImplementedError, match=what):
            HD.MultiScaleDiscriminator(**kw)
    ws, bs = DH.synth_plain(1)
    ok = torch.zeros(2, 1, 64)
    for d in (HD.DiscriminatorS(), HD.DiscriminatorS(use_spectral_norm=True, upsample_rates=[8, 8, 2, 2])):
        with pytest.raises(ValueError, match='no CPU path'):
            d(ok)
        with pytest.raises(ValueError, match=r'\[B\]\[1\]\[T\]'):
            d(torch.zeros(2, 2, 64))
        with pytest.raises(ValueError, match='float32'):
            d(ok.double())
        with pytest.raises(NotImplementedError, match='mel'):
            d(ok, torch.zeros(2, 80, 1))
    with pytest.raises(ValueError, match='no CPU path'):
        HD.disc_s_op(ok, ws, bs)
    with pytest.raises(ValueError, match=r'\[B\]\[1\]\[T\]'):
        HD.disc_s_op(torch.zeros(2, 64), ws, bs)
    with pytest.raises(ValueError, match='float32'):
        HD.disc_s_op(ok.half(), ws, bs)
    m = HD.MultiScaleDiscriminator()
    with pytest.raises(ValueError, match='T >= 4'):
        m(ok[:, :, :3], ok[:, :, :3])
    with pytest.raises(ValueError, match='no CPU path'):
        m(ok, ok)
    with pytest.raises(NotImplementedError, match='mel'):
        m(ok, ok, torch.zeros(2, 80, 1))
    assert HD.launch_count() == n0
    # the parameter checks, on the meta device: no storage, no launch
    xm = torch.zeros(2, 1, 64, device='meta')
    wm, bm = [w.to('meta') for w in ws], [b.to('meta') for b in bs]
    for bad_w, bad_b, what in ((wm[:7], bm[:7], 'eight weights'), (wm[:1] + [wm[1][:, :8]] + wm[2:], bm, r'weights\[1\]'),
                               (wm[:3] + [wm[3].double()] + wm[4:], bm, r'weights\[3\]'), (wm[:7] + [ws[7]], bm, r'weights\[7\]'),
                               (wm, bm[:5] + [bm[5][:3]] + bm[6:], r'biases\[5\]')):
        with pytest.raises(ValueError, match=what):
            HD._check_params(xm, bad_w, bad_b, 0.1, 'disc_s_op', HD._S_SHAPES, 'eight')
    with pytest.raises(ValueError, match='slope'):
        HD._check_params(xm, wm, bm, 1.0, 'disc_s_op', HD._S_SHAPES, 'eight')
    HD._check_params(xm, wm, bm[:2] + [None] + bm[3:], 0.1, 'disc_s_op', HD._S_SHAPES, 'eight')
    assert HD.launch_count() == n0


def test_keys_and_shapes_are_the_references():
    """the modules carry the reference's 80 state-dict entries in the reference's order; a strict load of the fixture's state succeeds"""
    from diffsinger_amd import MultiScaleDiscriminator, DiscriminatorS
    fx = DH.fixture()
    state = SH.fixture_inputs()[0]
    m = MultiScaleDiscriminator()
    sd = m.state_dict()
    assert list(sd) == fx['meta']['keys'] and len(sd) == 80
    assert [list(v.shape) for v in sd.values()] == fx['meta']['shapes']
    assert {k: tuple(v.shape) for k, v in sd.items()} == DH.module_shapes()
    assert list(sd) == list(DH.TwinMSD().state_dict())
    m.load_state_dict(state, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert len(m.meanpools) == 2 and not list(m.meanpools.parameters()) and not list(m.meanpools.buffers())
    assert len(m.discriminators[0].convs) == 7 and sum(p.numel() for p in m.discriminators[1].parameters()) == 9874306
    # the buffers are buffers, the rest parameters, as under torch's spectral_norm
    assert sorted(k for k, _ in m.named_buffers()) == sorted(k for k in sd if k.startswith('discriminators.0.') and (k.endswith('weight_u') or k.endswith('weight_v')))
    d = DiscriminatorS()
    d.load_state_dict({k[len('discriminators.1.'):]: v for k, v in state.items() if k.startswith('discriminators.1.')}, strict=True)
    d.remove_weight_norm()
    assert sorted(d.state_dict()) == sorted(p[len('discriminators.1.'):] + n for p in DH.prefixes(1) for n in ('weight', 'bias'))


@pytest.mark.parametrize('training', [False, True])
def test_spectral_holder_is_torchs_spectral_norm(training):
    """the holder's weight, its gradient and its buffers after two calls equal torch.nn.utils.spectral_norm's on the same state (CPU, float64)"""
    from diffsinger_amd.hifigan_disc import _SN
    gen = torch.Generator().manual_seed(3)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(12, 6, 5, groups=3)).double()
    h = _SN((6, 4, 5)).double()
    conv.weight_orig.data.copy_(torch.randn(6, 4, 5, generator=gen))
    h.load_state_dict(conv.state_dict(), strict=True)
    conv.train(training); h.train(training)
    x = torch.randn(2, 12, 9, generator=gen).double()
    for _ in range(2):
        want = conv(x)
        w = h.weight()
        got = torch.nn.functional.conv1d(x, w, h.bias, groups=3)
        assert float((got - want).abs().max()) <= 1e-13
    got.sum().backward(); want.sum().backward()
    assert float((h.weight_orig.grad - conv.weight_orig.grad).abs().max()) <= 1e-12
    for n in ('weight_u', 'weight_v'):
        assert float((getattr(h, n) - getattr(conv, n)).abs().max()) <= 1e-14
    assert torch.equal(h.weight_u, conv.state_dict()['weight_u']) or training


def test_recorded_spectral_buffers():
    """tests/golden/hifigan_msd_spectral.npz: discriminator 0's 16 buffers of the fixture's state as data - weight_u equal to the reference fixture's
    own recording bit for bit, every vector a unit vector to float32, laid over the regenerated state without touching anything else"""
    fx = DH.fixture()
    rec = SH.recorded_spectral()
    assert os.path.getsize(SH.SPECTRAL) <= 100 * 1000 and sorted(rec) == sorted(SH.spectral_keys()) and len(rec) == 16
    shapes = DH.module_shapes()
    for l, p in enumerate(DH.prefixes(0)):
        assert torch.equal(rec[p + 'weight_u'], torch.from_numpy(fx[f'eval/u{l}'])), l
        for n in ('weight_u', 'weight_v'):
            v = rec[p + n]
            assert v.dtype == torch.float32 and tuple(v.shape) == shapes[p + n] and abs(float(v.double().norm()) - 1.0) <= 1e-6, (p, n)
    plain, patched = DH.fixture_inputs()[0], SH.fixture_inputs()[0]
    assert list(plain) == list(patched)
    for k in plain:
        if k in rec:
            assert torch.equal(patched[k], rec[k]), k
        else:
            assert torch.equal(patched[k], plain[k]), k
