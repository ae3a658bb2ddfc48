"""CPU: the contract of FastSpeech2's counter-based training dropout (diffsinger_amd/dropout.py) that needs no device - the host scalars, the
refusals of the C entry points before any HIP call, and the statistics of the restated mask (tests/fs2_dropout_helpers.py) the GPU tests
compare the kernels with."""
import ctypes
import math

import numpy as np
import pytest
import torch

from diffsinger_amd import _lib, dropout
from tests import fs2_dropout_helpers as DH

SEED = 1234


def test_threshold_and_scale_of_the_shipped_rates():
    assert dropout.mask_threshold(0.1) == 429496730 == DH.thr_of(0.1)                  # round(0.1 * 2**32) = round(429496729.6)
    assert dropout.mask_threshold(0.5) == 2 ** 31 == DH.thr_of(0.5)
    assert dropout.mask_threshold(1 - 2.0 ** -40) == 2 ** 32 - 1                       # clamped: the compare stays 32-bit
    for p in (0.1, 0.5):
        s = dropout.mask_scale(p)
        assert s == float(np.float32(1.0 / (1.0 - p))) == float(DH.scale_of(p))
        assert np.float32(s) == s                                                      # float32 holds it exactly: the C float is this value
    assert dropout.mask_scale(0.5) == 2.0
    assert dropout.mask_scale(0.1) == float(np.float32(1.1111111111111112))


@pytest.mark.parametrize('p', [0, 1, -0.1])
def test_probabilities_outside_the_open_interval_are_value_errors(p):
    x = torch.zeros(8)
    with pytest.raises(ValueError):
        dropout.dropout_op(x, p, None)
    with pytest.raises(ValueError):
        dropout.dropout_add_keep_op(torch.zeros(1, 8, 32), torch.zeros(1, 8, 32), None, 5, p, None)
    with pytest.raises(ValueError):
        dropout.mask_threshold(p)


def test_disabled_by_default():
    assert dropout.current() is None


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    cell = (ctypes.c_uint64 * 2)(SEED, 0)
    a, st = ctypes.addressof(buf), ctypes.addressof(cell)
    thr, sc = dropout.mask_threshold(0.1), dropout.mask_scale(0.1)
    bad = [
        ('dsf_dropout', (None, a, 8, st, 0, thr, sc, None)),
        ('dsf_dropout', (a, None, 8, st, 0, thr, sc, None)),
        ('dsf_dropout', (a, a, 8, None, 0, thr, sc, None)),
        ('dsf_dropout', (a, a, 0, st, 0, thr, sc, None)),
        ('dsf_dropout', (a, a, -4, st, 0, thr, sc, None)),
        ('dsf_dropout', (a, a, 8, st, 0, 0, sc, None)),
        ('dsf_dropout_add_keep', (None, a, None, a, 1, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, None, None, a, 1, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, a, None, None, 1, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, a, None, a, 1, 1, 8, None, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, a, None, a, 0, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, a, None, a, 1, 0, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, a, None, a, 1, 1, 0, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep', (a, a, None, a, 1, 1, 8, st, 0, 0, sc, None)),
        ('dsf_dropout_add_keep_bwd', (None, None, a, a, 1, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep_bwd', (a, None, None, a, 1, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep_bwd', (a, None, a, None, 1, 1, 8, None, 0, thr, sc, None)),
        ('dsf_dropout_add_keep_bwd', (a, None, a, None, 1, 1, 0, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep_bwd', (a, None, a, None, 0, 1, 8, st, 0, thr, sc, None)),
        ('dsf_dropout_add_keep_bwd', (a, None, a, None, 1, 1, 8, st, 0, 0, sc, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)                            # DSD_ERR_INVALID, before any HIP call
        assert name.encode() in lib.dsd_last_error(), (name, lib.dsd_last_error())
    assert lib.dsf_dropout_grid_elements() >= 1024


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('step', [0, 1])
@pytest.mark.parametrize('site', [0, 1, 2])
def test_dropped_share_of_the_restated_mask(p, step, site):
    n = 32768
    share = 1.0 - DH.kept(SEED, step, site, n, p).mean()
    sigma = math.sqrt(p * (1 - p) / n)
    print(f'p={p} site={site} step={step}: dropped {share:.5f}, {(share - p) / sigma:+.2f} sigma')
    assert abs(share - p) <= 4 * sigma


def test_sites_and_steps_draw_independent_masks():
    n = 32768
    base = DH.kept(SEED, 0, 0, n, 0.5)
    for what, other in (('site 1', DH.kept(SEED, 0, 1, n, 0.5)), ('step 1', DH.kept(SEED, 1, 0, n, 0.5))):
        agree = float((base == other).mean())
        print(f'{what}: agrees with (site 0, step 0) on {agree:.4f}')
        assert 0.45 <= agree <= 0.55


def test_restated_ops_on_a_case_worked_by_hand():
    """The restatement itself: zero tail, keep, and the element order of the quads (element i draws word i & 3 of quad i >> 2)."""
    w = DH.words(SEED, 3, 7, 10)
    from oracle.philox_oracle import philox4x32_10
    for i in (0, 5, 9):
        q = philox4x32_10((np.uint32([i >> 2]), np.uint32([0]), np.uint32([7]), np.uint32([3])), (SEED, 0))
        assert int(w[i]) == int(q[i & 3][0])
    T, TS = 5, 32
    x = np.arange(2 * 8 * TS, dtype=np.float32).reshape(2, 8, TS) + 1
    res = -x / 3
    keep = np.ones((2, T), np.float32)
    keep[1, 2:] = 0
    y = DH.add_keep_ref(x, res, keep, T, SEED, 0, 0, 0.5)
    m = DH.kept(SEED, 0, 0, x.size, 0.5).reshape(x.shape)
    assert not y[:, :, T:].any() and not y[1, :, 2:].any()
    assert np.array_equal(y[0, :, :T], (res + np.where(m, x * np.float32(2), np.float32(0)))[0, :, :T])
    dx, dres = DH.add_keep_bwd_ref(x, keep, T, SEED, 0, 0, 0.5)
    assert not dres[:, :, T:].any() and not dx[:, :, T:].any() and not dres[1, :, 2:].any()
    assert np.array_equal(dx[0, :, :T], np.where(m, x * np.float32(2), np.float32(0))[0, :, :T])
