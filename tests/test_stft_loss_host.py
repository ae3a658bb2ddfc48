"""CPU: the host side of the STFT loss (diffsinger_amd/stft_loss.py, include/dsv.h section "STFT loss") - the float64 restatement the GPU
tests measure against agrees with what the reference's own module computed (tests/golden/stft_loss_ref.npz, written by
tools/make_golden_stft_loss.py), the public names are exported, and every refusal fires on a host without a GPU, before anything is launched."""
import os

import numpy as np
import pytest
import torch

from tests import stft_helpers as SH
from tests import stft_loss_helpers as LH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stft_loss_ref.npz')


def test_fixture_is_small_and_complete():
    assert os.path.getsize(GOLDEN) <= 160 * 1024
    g = np.load(GOLDEN)
    assert sorted(g.files) == ['g_mag', 'g_sc', 'mag', 'sc', 'x', 'y']
    assert g['x'].shape == g['y'].shape == g['g_sc'].shape == g['g_mag'].shape == (1, 8000)
    assert all(g[k].dtype == np.float32 for k in g.files)
    x, y = LH.signals('near')
    assert np.array_equal(g['x'], x[:1].numpy()) and np.array_equal(g['y'], y[:1].numpy())       # the 'near' pair of the GPU tests, first row


def test_float64_restatement_agrees_with_the_reference_module():
    g = np.load(GOLDEN)
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    (sc, mag), g_sc, g_mag = LH.grads_of(LH.ref_loss64, x.double(), y.double(), LH.RESOLUTIONS)
    (sc32, mag32), _, _ = LH.grads_of(LH.ref_loss32, x, y, LH.RESOLUTIONS)
    for name, got, got32, want in (('sc', float(sc), float(sc32), float(g['sc'])), ('mag', float(mag), float(mag32), float(g['mag']))):
        print(f'{name}: float64 restatement {got:.9f}, float32 restatement {got32:.9f}, reference module (float32) {want:.9f}: rel {abs(got - want) / want:.2e} (bound 1e-5)')
        assert abs(got - want) <= 1e-5 * want
        assert abs(got32 - want) <= 1e-5 * want
    # the gradients: printed, not bounded (1 / P amplifies the float32 forward's own error: GPU test 3 says why)
    for name, got, want in (('d sc/dx', g_sc, g['g_sc']), ('d mag/dx', g_mag, g['g_mag'])):
        err = float((got - torch.from_numpy(want).double()).abs().max())
        print(f'{name}: float64 restatement vs reference module (float32) max-abs {err:.3e} = {err / float(np.abs(want).max()):.2e} of max |.|')


def test_helper_transposes_agree():
    """vjp64 (autograd through torch.stft) and adjoint_matmul (explicit matrices) are the same operator, and it is the transpose."""
    for n_fft, hop, win, L, mode, center in ((256, 64, 256, 129, 'reflect', True), (256, 64, 200, 700, 'constant', True), (512, 128, 512, 900, 'reflect', False)):
        x = SH.make_signal(L, seed=3, batch=2).double()
        S = torch.view_as_real(SH.ref_stft64(x, n_fft, hop, win, center, mode))
        G = torch.randn(S.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        a = LH.vjp64(G, L, n_fft, hop, win, center, mode)
        b = LH.adjoint_matmul(G, L, n_fft, hop, win, center, mode, dtype=torch.float64)
        lhs, rhs = float((S * G).sum()), float((x * a).sum())
        assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
        assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())      # the matrix form rounds its basis to float32


def test_public_names_are_exported():
    import diffsinger_amd
    for name in ('STFTLoss', 'MultiResolutionSTFTLoss', 'stft_adjoint_op', 'spectral_loss_op'):
        assert name in diffsinger_amd.__all__
        assert callable(getattr(diffsinger_amd, name))
    from diffsinger_amd import _lib
    for name in ('dsv_stft_make_adjoint_basis', 'dsv_stft_adjoint_workspace_floats', 'dsv_stft_adjoint', 'dsv_spectral_loss_workspace_floats',
                 'dsv_spectral_loss', 'dsv_spectral_loss_backward'):
        assert name in _lib.SYMBOLS_VOC


def test_constructor_signatures_are_the_references():
    import inspect
    from diffsinger_amd import MultiResolutionSTFTLoss, STFTLoss
    p = inspect.signature(STFTLoss.__init__).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:5]] == [('fft_size', 1024), ('shift_size', 120), ('win_length', 600), ('window', 'hann_window')]
    p = inspect.signature(MultiResolutionSTFTLoss.__init__).parameters
    assert [k for k in list(p)[1:5]] == ['fft_sizes', 'hop_sizes', 'win_lengths', 'window']
    assert [list(p[k].default) for k in ('fft_sizes', 'hop_sizes', 'win_lengths')] == [[1024, 2048, 512], [120, 240, 50], [600, 1200, 240]]
    m = MultiResolutionSTFTLoss()
    assert [(f.fft_size, f.shift_size, f.win_length) for f in m.stft_losses] == list(LH.RESOLUTIONS)
    assert not list(m.state_dict())                                           # like the reference's: nothing to load or save


def test_refusals_fire_without_a_gpu():
    from diffsinger_amd import MultiResolutionSTFTLoss, STFTLoss, spectral_loss_op, stft_adjoint_op
    with pytest.raises((ValueError, NotImplementedError), match='hann_window'):
        STFTLoss(window='hamming_window')
    with pytest.raises((ValueError, NotImplementedError), match='hann_window'):
        MultiResolutionSTFTLoss(window='blackman_window')
    with pytest.raises(NotImplementedError, match='use_mel_loss'):
        STFTLoss(use_mel_loss=True)
    with pytest.raises(NotImplementedError, match='use_mel_loss'):
        MultiResolutionSTFTLoss(use_mel_loss=True)
    with pytest.raises(ValueError, match='n_fft=1000'):
        STFTLoss(1000, 100, 500)
    with pytest.raises(ValueError, match='n_fft=4096'):
        MultiResolutionSTFTLoss([1024, 4096], [120, 480], [600, 2400])
    with pytest.raises(ValueError, match='one entry per resolution'):
        MultiResolutionSTFTLoss([1024, 512], [120], [600, 240])
    one, multi = STFTLoss(), MultiResolutionSTFTLoss()
    x = torch.zeros(2, 4000)
    for crit, T in ((one, 512), (multi, 1024)):                              # reflect padding of n_fft / 2 needs T > n_fft / 2
        with pytest.raises(ValueError, match='reflect padding'):
            crit(x[:, :T], x[:, :T])
    for crit in (one, multi):
        with pytest.raises(ValueError, match=r'\[B\]\[T\]'):
            crit(x, x[:, :3999])
        with pytest.raises(ValueError, match=r'\[B\]\[T\]'):
            crit(x[0], x[0])
        with pytest.raises(ValueError, match='different devices'):
            crit(x, torch.zeros(2, 4000, device='meta'))
        with pytest.raises(NotImplementedError, match='target'):
            crit(x, x.clone().requires_grad_(True))
        with pytest.raises(NotImplementedError, match='no CPU path'):
            crit(x, x)
    S = torch.zeros(1, 129, 9, dtype=torch.complex64)
    with pytest.raises(ValueError, match='share layout and shape'):
        spectral_loss_op(S, S[:, :, :8])
    with pytest.raises(NotImplementedError, match='target'):
        spectral_loss_op(S, S.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match='no CPU path'):
        spectral_loss_op(S, S)
    with pytest.raises(ValueError, match='n_fft=1000'):
        stft_adjoint_op(S, 512, n_fft=1000, hop=64)
    with pytest.raises(ValueError, match='spectrum must be'):
        stft_adjoint_op(S[:, :128], 512, n_fft=256, hop=64)
    with pytest.raises(ValueError, match='9 frames, the cotangent 8'):
        stft_adjoint_op(S[:, :, :8], 512, n_fft=256, hop=64)
    with pytest.raises(ValueError, match='reflect padding'):
        stft_adjoint_op(S, 128, n_fft=256, hop=64, pad_mode='reflect')
    with pytest.raises(RuntimeError, match='no CPU path'):
        stft_adjoint_op(S, 512, n_fft=256, hop=64)


def test_abi_sizes_and_refusals_without_a_device():
    """What the C ABI answers on the host alone: sizes, and the argument checks that come before any launch."""
    from diffsinger_amd import _lib
    lib = _lib.load()
    assert lib.dsv_stft_basis_floats(1024, 2) == 1024 * 1024 and lib.dsv_stft_basis_floats(768, 2) == -1 and lib.dsv_stft_basis_floats(1024, 3) == -1
    assert lib.dsv_stft_basis_floats(1024, 0) == 1024 * 1024 and lib.dsv_stft_basis_floats(1024, 1) == 1024 * 1024 + 1024       # unchanged
    assert lib.dsv_stft_adjoint_workspace_floats(2, 67, 1024) == 2 * 67 * 1024 and lib.dsv_stft_adjoint_workspace_floats(2, 67, 1000) == -1
    assert lib.dsv_spectral_loss_workspace_floats(0) == -1 and lib.dsv_spectral_loss_workspace_floats(1) == 14
    assert lib.dsv_spectral_loss_workspace_floats(10 ** 9) == 2 * (4 + 3 * 1024)
    assert lib.dsv_stft_make_adjoint_basis(768, 768, None, None) == -1 and b'n_fft=768' in lib.dsd_last_error()
    assert lib.dsv_stft_make_adjoint_basis(1024, 1025, None, None) == -1 and b'win_length=1025' in lib.dsd_last_error()
    assert lib.dsv_stft_make_adjoint_basis(1024, 600, None, None) == -1 and b'null' in lib.dsd_last_error()
    assert lib.dsv_stft_adjoint(None, None, None, None, 1, 4096, 1024, 256, 512, 512, 0, None) == -1 and b'null' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss(None, None, None, None, 10, None) == -1 and b'null' in lib.dsd_last_error()
    assert lib.dsv_spectral_loss_backward(None, None, None, None, None, 10, None) == -1 and b'null' in lib.dsd_last_error()
