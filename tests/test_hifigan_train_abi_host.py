"""CPU: the C ABI of HiFi-GAN generator training (include/dsv.h section "HiFi-GAN generator training", csrc/hifigan_train_abi.hpp) without a
device: every declared symbol is exported and bound, every sizing function equals an independent formula at the test shapes and at the training
shape of configs/tts/hifigan.yaml (c0 = 128, rates [8, 8, 2, 2], B = 16, 8192 samples), and every entry point refuses nulls, bad shapes and
too-short workspaces with an error string BEFORE any launch (these calls run on a machine without a GPU)."""
import ctypes

import pytest
import torch

from diffsinger_amd import _lib
from tests.test_abi import _header_symbols


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def ls(L):
    return (L + 31) // 32 * 32


def test_every_declared_symbol_is_exported_and_bound(lib):
    declared = [s for s in _header_symbols('dsv.h', 'dsv_') if s.startswith('dsv_hgt_')]
    assert len(declared) == 12 and len(set(declared)) == 12
    for name in declared:
        assert name in _lib.SYMBOLS_VOC, name
        assert hasattr(lib, name), name
    assert sorted(s for s in _lib.SYMBOLS_VOC if s.startswith('dsv_hgt_')) == sorted(declared)


def wgrad_floats(S, B, L, Co, Ci, K, up):
    return B * ((L + S - 1) // S) * (Co * up) * (Ci * K)


def test_sizing_functions_equal_an_independent_formula(lib):
    S = lib.dsv_hgt_wgrad_split()
    assert S >= 32 and S % 32 == 0
    q, a, bs = lib.dsv_hgt_wgrad_workspace_floats, lib.dsv_hgt_act_floats, lib.dsv_hgt_bias_workspace_floats
    bias_floats = lambda B, C, L: 2 * C * B * ((L + 1023) // 1024)                      # noqa: E731  (float64 partials per 1024-sample chunk)
    # the operator tests' shapes (B, C, K, dil, L) and (B, Ci -> Co, u, polyphase taps 3, L_in)
    for B, C, K, L in [(2, 8, 11, 20), (1, 16, 7, 100), (3, 32, 3, S + 33), (2, 64, 11, 130), (1, 128, 7, 40), (1, 8, 3, 1061), (1, 16, 7, 90)]:
        assert q(B, L, C, C, K, 1) == wgrad_floats(S, B, L, C, C, K, 1)
        assert q(B, L, 1, C, 7, 1) == wgrad_floats(S, B, L, 1, C, 7, 1)
        assert a(B, C, L) == B * C * ls(L)
        assert bs(B, C, L) == bias_floats(B, C, L) and bs(B, 1, L) == bias_floats(B, 1, L)
    for B, Ci, Co, u, L in [(2, 128, 64, 8, 9), (1, 64, 32, 8, 70), (2, 32, 16, 2, 130), (1, 16, 8, 2, S // 2 + 17), (1, 32, 16, 4, 33)]:
        assert q(B, L, Co, Ci, 3, u) == wgrad_floats(S, B, L, Co, Ci, 3, u)
        assert a(B, Co, L * u) == B * Co * ls(L * u) and bs(B, Co, L * u) == bias_floats(B, Co, L * u)
    # the training shape: 16 x 8192 samples = 32 frames, channels 128 -> 64 -> 32 -> 16 -> 8 at 256 / 2048 / 4096 / 8192 samples
    B, T = 16, 32
    assert q(B, T, 128, 80, 7, 1) == wgrad_floats(S, B, T, 128, 80, 7, 1)
    L, ch, biggest = T, 128, 0
    for u in (8, 8, 2, 2):
        assert q(B, L, ch // 2, ch, 3, u) == wgrad_floats(S, B, L, ch // 2, ch, 3, u)
        biggest = max(biggest, q(B, L, ch // 2, ch, 3, u))
        L, ch = L * u, ch // 2
        for K in (3, 7, 11):
            assert q(B, L, ch, ch, K, 1) == wgrad_floats(S, B, L, ch, ch, K, 1)
            biggest = max(biggest, q(B, L, ch, ch, K, 1))
        assert a(B, ch, L) == B * ch * ls(L) < 2 ** 31 and bs(B, ch, L) == bias_floats(B, ch, L)
    assert L == 8192 and q(B, L, 1, ch, 7, 1) == wgrad_floats(S, B, L, 1, ch, 7, 1)
    assert biggest * 4 < 2 ** 31                                     # nothing at the training shape comes near a 32-bit index
    # a length only 64 bits hold
    assert q(65535, 1 << 20, 1024, 1024, 64, 1) == wgrad_floats(S, 65535, 1 << 20, 1024, 1024, 64, 1) > 2 ** 40
    assert a(65535, 1024, 1 << 30) == 65535 * 1024 * (1 << 30)
    # refused shapes
    assert q(0, 8, 8, 8, 3, 1) == -1 and q(65536, 8, 8, 8, 3, 1) == -1 and q(1, 0, 8, 8, 3, 1) == -1 and q(1, 8, 0, 8, 3, 1) == -1
    assert q(1, 8, 8, 1025, 3, 1) == -1 and q(1, 8, 8, 8, 0, 1) == -1 and q(1, 8, 8, 8, 3, 0) == -1 and q(1, (1 << 30), 8, 8, 3, 2) == -1
    assert bs(16, 1, 8192) == 2 * 16 * 8 and bs(2, 64, 1024) == 2 * 64 * 2 and bs(2, 64, 1025) == 2 * 64 * 2 * 2
    assert bs(0, 8, 8) == -1 and bs(1, 0, 8) == -1 and bs(1, 1025, 8) == -1 and bs(1, 8, 0) == -1
    assert a(0, 8, 8) == -1 and a(1, 0, 8) == -1 and a(1, 8, 0) == -1 and a(65536, 8, 8) == -1


def refused(lib, name, *args):
    assert getattr(lib, name)(*args, None) == -1, name
    msg = lib.dsd_last_error()
    assert name.encode() in msg, (name, msg)
    return msg


def test_entry_points_refuse_before_any_launch(lib):
    buf = torch.zeros(1 << 16)                                       # host memory: a call that launched would not return an error string
    p = buf.data_ptr()
    S = lib.dsv_hgt_wgrad_split()
    # nulls
    refused(lib, 'dsv_hgt_conv_dgrad', None, None, None, None, None, None, 1, 8, 8, 3, 1, 1, 8, 0.1, 1.0)
    refused(lib, 'dsv_hgt_conv_wgrad', None, None, None, 0, None, 1, 8, 8, 3, 1, 1, 8, 1, 0.1)
    refused(lib, 'dsv_hgt_bias_grad', None, None, 0, None, 1, 8, 8)
    refused(lib, 'dsv_hgt_upsample_dgrad', None, None, None, None, 1, 16, 8, 2, 4, 8, 0.1, 1.0)
    refused(lib, 'dsv_hgt_tanh_backward', None, None, None, 1, 8)
    refused(lib, 'dsv_hgt_noise_conv_backward', None, None, None, None, 0, None, None, None, 1, 8, 4, 2, 1, 16, 8, 1)
    refused(lib, 'dsv_hgt_source_mix', None, None, None, None, 1, 4, 4, 9, 0.1, 0.003, 0.0)
    refused(lib, 'dsv_hgt_source_backward', None, None, None, None, None, 1, 8, 9)
    # bad shapes: batch, length, channels, reach beyond +-48 samples, in-place, zero divisor
    for B, Cg, C, K, pad, dil, L, div in [(0, 8, 8, 3, 1, 1, 8, 1.0), (65536, 8, 8, 3, 1, 1, 8, 1.0), (1, 8, 8, 3, 1, 1, 0, 1.0), (1, 0, 8, 3, 1, 1, 8, 1.0),
                                          (1, 8, 1025, 3, 1, 1, 8, 1.0), (1, 8, 8, 11, 50, 10, 8, 1.0), (1, 8, 8, 3, 3, 1, 8, 1.0), (1, 8, 8, 3, 1, 1, 8, 0.0)]:
        refused(lib, 'dsv_hgt_conv_dgrad', p, p + 4096, p + 8192, None, None, p + 16384, B, Cg, C, K, pad, dil, L, 0.1, div)
    refused(lib, 'dsv_hgt_conv_dgrad', p, p + 4096, p + 8192, None, None, p, 1, 8, 8, 3, 1, 1, 8, 0.1, 1.0)
    for B, Co, Ci, K, pad, dil, L, up in [(0, 8, 8, 3, 1, 1, 8, 1), (1, 8, 8, 3, 1, 1, 0, 1), (1, 1025, 8, 3, 1, 1, 8, 1), (1, 8, 8, 65, 32, 1, 8, 1),
                                          (1, 8, 8, 11, 50, 10, 8, 1), (1, 8, 8, 3, 1, 1, 8, 0), (1, 8, 8, 3, 1, 1, 1 << 30, 2)]:
        refused(lib, 'dsv_hgt_conv_wgrad', p, p, p, 1 << 40, p, B, Co, Ci, K, pad, dil, L, up, 0.1)
    # a workspace one float short of the library's own requirement
    need = lib.dsv_hgt_wgrad_workspace_floats(2, S + 33, 16, 8, 3, 2)
    msg = refused(lib, 'dsv_hgt_conv_wgrad', p, p, p, need - 1, p, 2, 16, 8, 3, 1, 1, S + 33, 2, 0.1)
    assert str(need).encode() in msg and str(need - 1).encode() in msg
    refused(lib, 'dsv_hgt_conv_wgrad', p, p, p, 0, p, 1, 8, 8, 3, 1, 1, 8, 1, 0.1)
    refused(lib, 'dsv_hgt_conv_wgrad', p, p, p, -5, p, 1, 8, 8, 3, 1, 1, 8, 1, 0.1)
    refused(lib, 'dsv_hgt_bias_grad', p, p, 1 << 40, p, 1, 0, 8)
    refused(lib, 'dsv_hgt_bias_grad', p, p, 1 << 40, p, 65536, 8, 8)
    bneed = lib.dsv_hgt_bias_workspace_floats(2, 8, 1061)
    msg = refused(lib, 'dsv_hgt_bias_grad', p, p, bneed - 1, p, 2, 8, 1061)
    assert str(bneed).encode() in msg
    refused(lib, 'dsv_hgt_bias_grad', p, None, bneed, p, 2, 8, 1061)
    refused(lib, 'dsv_hgt_bias_grad', p, p + 4, bneed, p, 2, 8, 1061)                       # float64 partials: 8-byte alignment
    for Ci, Co, up, K, L, div in [(0, 8, 2, 4, 8, 1.0), (16, 8, 0, 4, 8, 1.0), (16, 8, 2, 5, 8, 1.0), (16, 8, 4, 2, 8, 1.0), (16, 8, 2, 4, 1 << 30, 1.0),
                                  (16, 8, 2, 4, 8, 0.0)]:
        refused(lib, 'dsv_hgt_upsample_dgrad', p, p + 4096, p + 8192, p + 16384, 1, Ci, Co, up, K, L, 0.1, div)
    refused(lib, 'dsv_hgt_tanh_backward', p, p, p, 1, 0)
    # noise convolution: L_out must be the convolution's own output length
    refused(lib, 'dsv_hgt_noise_conv_backward', p, p, p, p, 1 << 40, p, p, p, 1, 8, 4, 2, 1, 16, 9, 1)
    refused(lib, 'dsv_hgt_noise_conv_backward', p, p, p, p, 1 << 40, p, p, p, 1, 0, 4, 2, 1, 16, 8, 1)
    refused(lib, 'dsv_hgt_noise_conv_backward', p, p, p, p, lib.dsv_hgt_bias_workspace_floats(1, 8, 8) - 1, p, p, p, 1, 8, 4, 2, 1, 16, 8, 1)
    refused(lib, 'dsv_hgt_source_mix', p, p, p, p, 1, 4, 4, 65, 0.1, 0.003, 0.0)
    refused(lib, 'dsv_hgt_source_mix', p, p, p, p, 1, 1 << 20, 1 << 12, 9, 0.1, 0.003, 0.0)
    refused(lib, 'dsv_hgt_source_backward', p, p, p, p, p, 1, 8, 0)


def test_forward_train_refuses_what_it_does_not_cover_without_a_device():
    from diffsinger_amd.vocoder import HifiGanGenerator
    from tests import hifigan_train_helpers as TH
    gen = HifiGanGenerator(TH.config(upsample_initial_channel=16))
    x = torch.zeros(1, 80, 4)
    with pytest.raises(NotImplementedError, match='no gradient with respect to x'):
        gen.forward_train(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='no CPU path'):
        gen.forward_train(x)
    nsf = HifiGanGenerator(TH.config(use_pitch_embed=True, upsample_initial_channel=16))
    with pytest.raises(NotImplementedError, match='no gradient with respect to f0'):
        nsf.forward_train(x, torch.zeros(1, 4, requires_grad=True))
    with pytest.raises(NotImplementedError, match='no gradient with respect to noise'):
        nsf.forward_train(x, torch.zeros(1, 4), noise=torch.zeros(1, 4 * 64, 9, requires_grad=True))


def test_parameter_layout_covers_every_parameter_in_both_forms():
    from diffsinger_amd.hifigan_train import param_layout, polyphase_taps
    from diffsinger_amd.vocoder import HifiGanGenerator, polyphase_weight
    from tests import hifigan_train_helpers as TH
    for over in (dict(), dict(use_pitch_embed=True), dict(resblock='2')):
        h = TH.config(**over)
        gen = HifiGanGenerator(h)
        for removed in (False, True):
            if removed:
                gen.remove_weight_norm()
            assert {k: tuple(v.shape) for k, v in gen.state_dict().items()} == TH.module_shapes(h, weight_norm_on=not removed)
            prefixes = [p for p, _ in param_layout(h)]
            assert sorted(prefixes) == sorted(p for p, _, _ in TH.module_prefixes(h))
            ps = gen._train_params()
            assert len(ps) == 2 * len(prefixes)
            for n, p in enumerate(prefixes):
                assert tuple(ps[2 * n].shape) == dict((q, s) for q, s, _ in TH.module_prefixes(h))[p]
    # the tap map the weight gradient is gathered through is polyphase_weight's own
    for k, u in ((16, 8), (8, 4), (4, 2), (8, 8), (6, 2)):
        w = torch.arange(1, 2 * 3 * k + 1, dtype=torch.float32).reshape(2, 3, k)
        wp, pad = polyphase_weight(w, u, (k - u) // 2)
        r_of, t_of, kk, ppad = polyphase_taps(k, u)
        assert (kk, ppad) == (wp.shape[2], pad)
        v = wp.reshape(3, u, 2, kk)
        for j in range(k):
            assert torch.equal(v[:, r_of[j], :, t_of[j]], w[:, :, j].t())
        assert int((wp != 0).sum()) == w.numel()
