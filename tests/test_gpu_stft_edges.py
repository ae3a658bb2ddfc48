"""GPU: the STFT family (include/dsv.h section "STFT"; k_stft<MODE, GT> and k_istft_ola in csrc/voc_stft.hpp, planned by csrc/voc_stft_abi.hpp) at
the hops, frame counts and signal ends it runs at - the cases, float64 restatements and bounds of tests/stft_edge_helpers.py, which
tests/test_stft_edges_host.py replays on the CPU with restated bugs.

What tests/test_gpu_stft.py leaves open and this file closes: hops that are no multiple of 64 (the stft-loss resolutions, odd, 1, n_fft, larger
than the planned chunk), frame counts at the 64-frame workgroup seam, the unsplit (grid.z = 1) launch of >= 512 workgroups - the only one in
which a workgroup loops over more than one row group (n_fft >= 512), forward and inverse - the inverse over its WHOLE length (both
ends, center=False, gaps in the window sum, L_out past the signal, frame_counts, the windowed frames in the workspace), the subtracted spectrum
itself, mel bases that weigh bin 0 and the Nyquist bin (M = 1 .. 128, one-hot rows), and `lengths` outside [0, L] or no longer than the reflect
padding.

No bound is measured on the device: spectra, magnitudes and log-mels 2 x the CPU float32 yardstick on the case's own input; the inverse by the
per-sample condition of stft_edge_helpers.inverse_bound; exact zeros and bitwise equalities where the header promises them.  Every test prints
its measured maximum next to its bound (recorded in profiles/stft_edges_pytest_gpu.txt)."""
import pytest
import torch

from diffsinger_amd import _lib
from diffsinger_amd import stft as ST
from tests import stft_edge_helpers as EH
from tests import stft_helpers as SH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    return a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize('n_fft,hop,win', EH.FORWARD_GEOMS)
def test_forward_hops_and_frame_counts(n_fft, hop, win):
    KC, RL = EH.plan(n_fft, hop)
    worst = 0.0
    for T, L, center, mode in EH.forward_cases(n_fft, hop, win):
        c = EH.forward_case(n_fft, hop, win, T, L, center, mode)
        got = ST.stft_op(c['wav'].to(DEV), n_fft=n_fft, hop=hop, win_length=win, center=center, pad_mode=mode)
        assert got.shape == c['want'].shape and got.dtype == torch.complex64
        err = EH.cerr(got, c['want'])
        worst = max(worst, err / (2 * c['yard']))
        print(f'stft {n_fft}/{hop}/{win} L={L} {mode} center={int(center)}: {T} frames x {EH.ROWS} rows, max-abs err {err:.3e}, bound {2 * c["yard"]:.3e} (2 x CPU fp32 yardstick)')
        assert err <= 2 * c['yard'], (T, L, center, mode, err, c['yard'])
    print(f'stft {n_fft}/{hop}/{win} (KC={KC}, RL={RL}): largest share of the bound {worst:.2f}')


@pytest.mark.parametrize('n_fft,hop,win,B,T', EH.UNSPLIT_CASES)
def test_forward_unsplit_launch(n_fft, hop, win, B, T):
    """>= 512 workgroups: stft_zsplit returns grid.z = 1.  At n_fft = 256 there is one row group, so this is the plan of every call (rows are
    independent of the batch, nothing more).  At 512/128 (two groups, one chunk) and 2048/300 (eight groups, chunks of 256) it is the ONLY
    launch in which a workgroup loops over row groups - reusing the staged window, or staging every chunk again behind the barrier - while the
    B = 1 call of the same samples runs one group per grid.z and never loops.  Both must carry the same bits
    (tests/test_stft_edges_host.py asserts these plans from the restated stft_zsplit)."""
    z_big, z_solo, groups = EH.zsplit(T, B, n_fft), EH.zsplit(T, 1, n_fft), EH.row_groups(n_fft)
    assert z_big == 1 and z_solo == groups
    L = n_fft + hop * (T - 1)
    wav = SH.make_signal(L, seed=12, batch=B)
    dev = wav.to(DEV)
    got = ST.stft_op(dev, n_fft=n_fft, hop=hop, win_length=win, center=False)
    assert got.shape == (B, n_fft // 2 + 1, T)
    rows = [0, B // 2 - 1, B - 1]
    want = SH.ref_stft64(wav[rows], n_fft, hop, win, center=False)
    yard = EH.cerr(SH.yardstick32(wav[rows], n_fft, hop, win, center=False), want)
    err = EH.cerr(got[rows], want)
    print(f'unsplit launch {n_fft}/{hop}/{win} B={B} x {T} frames (grid.z 1, {groups} row group(s) per workgroup), rows {rows}: max-abs err {err:.3e}, '
          f'bound {2 * yard:.3e}; share {err / (2 * yard):.2f}')
    assert err <= 2 * yard
    for b in range(B):
        assert _bits(ST.stft_op(dev[b:b + 1], n_fft=n_fft, hop=hop, win_length=win, center=False), got[b:b + 1]), b
    print(f'unsplit launch {n_fft}/{hop}/{win}: all {B} rows carry the bits of their B = 1 call (grid.z {z_solo}, one row group per workgroup)')


def _istft_raw(S, n_fft, hop, win, center, length, fc):
    """dsv_istft through the C ABI: (wav [B][length], windowed frames [B][nF][n_fft] read from the caller's workspace), both pre-filled with NaN"""
    lib = _lib.load()
    s = torch.view_as_real(S.to(torch.complex64).to(DEV).contiguous())
    B, _, T, _ = s.shape
    _, inv = ST.bases(DEV, n_fft, win)
    ws = torch.full((int(lib.dsv_istft_workspace_floats(B, T, n_fft)),), float('nan'), device=DEV)
    out = torch.full((B, length), float('nan'), device=DEV)
    fcs = torch.tensor(fc, dtype=torch.int32, device=DEV) if fc is not None else None
    _lib.check(lib.dsv_istft(s.data_ptr(), fcs.data_ptr() if fcs is not None else None, inv.data_ptr(), ws.data_ptr(), out.data_ptr(), B, T, length,
                             n_fft, hop, int(center), torch.cuda.current_stream().cuda_stream), 'dsv_istft')
    torch.cuda.synchronize()
    return out.cpu(), ws.view(B, T, n_fft).cpu()


@pytest.mark.parametrize('n_fft,hop,win', EH.INVERSE_GEOMS)
def test_inverse_whole_length(n_fft, hop, win):
    w_fr = w_out = 0.0
    for T in EH.INVERSE_FRAMES:
        dirty, clean = EH.inverse_case(n_fft, hop, win, T)
        for center in (True, False):
            for length, fc in EH.inverse_calls(n_fft, hop, T, center):
                ref = EH.inverse_refs(dirty, n_fft, hop, win, center, length, fc)
                out, frames = _istft_raw(dirty, n_fft, hop, win, center, length, fc)
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(frames).all())             # every element written
                e_fr, share, bad = EH.judge_inverse(ref, frames.numpy(), out.numpy())
                w_fr, w_out = max(w_fr, e_fr / (2 * ref['Y'])), max(w_out, share)
                print(f'istft {n_fft}/{hop}/{win} T={T} center={int(center)} L_out={length} frame_counts={fc}: frames max-abs err {e_fr:.3e}, bound {2 * ref["Y"]:.3e}; '
                      f'output measured/bound {share:.3f} (worst sample), {bad} sample(s) not exactly 0 where the window sum is 0 or the signal has ended')
                assert e_fr <= 2 * ref['Y'] and share <= 1 and bad == 0, (T, center, length, fc, e_fr, ref['Y'], share, bad)
                # the imaginary parts of bins 0 and n_fft / 2 do not change a bit; the operator of diffsinger_amd.stft is this call
                out0, frames0 = _istft_raw(clean, n_fft, hop, win, center, length, fc)
                assert torch.equal(out0, out) and torch.equal(frames0, frames)
                op = ST.istft_op(dirty.to(DEV), n_fft=n_fft, hop=hop, win_length=win, center=center, length=length, frame_counts=fc)
                assert torch.equal(op.cpu(), out)
    print(f'istft {n_fft}/{hop}/{win}: largest share of the bound - windowed frames {w_fr:.2f}, output {w_out:.3f}')


def test_inverse_unsplit_launch():
    """The inverse product (k_stft<2, 2>) with >= 512 workgroups at n_fft = 512: grid.z = 1, every workgroup loops over both row groups and
    stages both chunks of 256 spectrum slots again for the second - against float64 on three rows, and bitwise against the B = 1 calls, which
    run one group per grid.z."""
    n_fft, hop, win, B, T = EH.UNSPLIT_INVERSE
    assert EH.zsplit(T, B, n_fft) == 1 and EH.zsplit(T, 1, n_fft) == EH.row_groups(n_fft) == 2 and EH.plan(n_fft, n_fft)[0] < n_fft
    wav = SH.make_signal(n_fft + hop * (T - 1), seed=13, batch=B)
    S = SH.ref_stft64(wav, n_fft, hop, win, center=False).to(torch.complex64)
    length = hop * (T - 1)
    out, frames = _istft_raw(S, n_fft, hop, win, True, length, None)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(frames).all())
    rows = [0, B // 2 - 1, B - 1]
    ref = EH.inverse_refs(S[rows], n_fft, hop, win, True, length, None)
    e_fr, share, bad = EH.judge_inverse(ref, frames[rows].numpy(), out[rows].numpy())
    print(f'unsplit inverse {n_fft}/{hop}/{win} B={B} x {T} frames (grid.z 1, 2 row groups per workgroup), rows {rows}: frames max-abs err {e_fr:.3e}, '
          f'bound {2 * ref["Y"]:.3e}; output measured/bound {share:.3f}, {bad} sample(s) not exactly 0 that must be')
    assert e_fr <= 2 * ref['Y'] and share <= 1 and bad == 0
    for b in range(B):
        o, f = _istft_raw(S[b:b + 1], n_fft, hop, win, True, length, None)
        assert torch.equal(o, out[b:b + 1]) and torch.equal(f, frames[b:b + 1]), b
    print(f'unsplit inverse {n_fft}/{hop}/{win}: all {B} rows carry the bits of their B = 1 call (grid.z 2), windowed frames and output')


@pytest.mark.parametrize('n_fft,hop,win', EH.SUBTRACT_GEOMS)
def test_subtraction_on_the_spectrum(n_fft, hop, win):
    c = EH.subtract_case(n_fft, hop, win)
    dev = c['wav'].to(DEV)
    plain = ST.stft_op(dev, n_fft=n_fft, hop=hop, win_length=win)
    worst = 0.0
    for v in c['vs']:
        got = ST.stft_op(dev, n_fft=n_fft, hop=hop, win_length=win, subtract=v)
        share, bad = EH.judge_subtract(got, c, v)
        worst = max(worst, share)
        print(f'subtraction {n_fft}/{hop}/{win} v={v:.4g}: measured/bound {share:.2f} (worst element; bound 2 x {c["yard"]:.3e} + 4 u |S|), '
              f'{bad} element(s) not exactly 0 that must be')
        assert share <= 1 and bad == 0
    assert _bits(ST.stft_op(dev, n_fft=n_fft, hop=hop, win_length=win, subtract=0.0), plain)              # v = 0: the bits of the unfiltered call
    assert not bool(torch.view_as_real(ST.stft_op(dev, n_fft=n_fft, hop=hop, win_length=win, subtract=c['vs'][-1])).any())   # v above every magnitude
    print(f'subtraction {n_fft}/{hop}/{win}: largest share of the bound {worst:.2f}')


@pytest.mark.parametrize('flavour', ['pwg', 'hifigan'])
@pytest.mark.parametrize('n_fft,hop,win', EH.MEL_GEOMS)
def test_logmel_dense_basis(flavour, n_fft, hop, win):
    """A basis that weighs every bin, bin 0 and the Nyquist bin included (the shipped filterbanks weigh both with exactly 0), at Mt = 1, 2, 3, 4
    tiles of mel rows, 65 frames and one.  Log-domain comparison under the condition of tests/test_gpu_stft.py: float64 mel >= 1e-3."""
    worst = 0.0
    for T in (65, 1):
        over, wav = EH.mel_signal(flavour, n_fft, hop, T)
        name = flavour + ''.join(f' {k}={v}' for k, v in over.items())
        for M in EH.MEL_ROWS:
            basis = EH.dense_basis(M, n_fft)
            r = EH.logmel_refs(wav, basis, flavour, over, n_fft, hop, win)
            want, want_mel, want_mag, yard, yard_mag = r['want'], r['mel'], r['mag'], r['yard'], r['yard_mag']
            assert want.shape[1] == T and float(want_mel.min()) >= 1e-3, (want.shape, float(want_mel.min()))
            bdev = torch.from_numpy(basis).to(DEV)
            got, lin = ST.logmel_op(wav.to(DEV), bdev, n_fft=n_fft, hop=hop, win_length=win, flavour=flavour, return_linear=True, **over)
            assert got.shape == want.shape and lin.shape == want_mag.shape
            err = float((got.cpu().double() - want).abs().max())
            err_mag = float((lin.cpu().double() - want_mag).abs().max())
            worst = max(worst, err / (2 * yard), err_mag / (2 * yard_mag))
            print(f'logmel {name} {n_fft}/{hop}/{win} M={M} T={T} x {wav.shape[0]} rows: log-domain err {err:.3e}, bound {2 * yard:.3e}; magnitude err {err_mag:.3e}, '
                  f'bound {2 * yard_mag:.3e}; min mel {float(want_mel.min()):.3f}')
            assert err <= 2 * yard and err_mag <= 2 * yard_mag, (T, M, err, yard, err_mag, yard_mag)
            only = ST.logmel_op(wav.to(DEV), bdev, n_fft=n_fft, hop=hop, win_length=win, flavour=flavour, **over)
            assert torch.equal(only, got)                                     # the optional output does not change the mel
    print(f'logmel {flavour} {n_fft}/{hop}/{win}, dense basis: largest share of the bound {worst:.2f}')


@pytest.mark.parametrize('flavour', ['pwg', 'hifigan'])
def test_logmel_one_hot_basis(flavour):
    """Row m selects bin m (first call) / bin m + 1 (second call): the mel of a row IS that bin's magnitude, so the log-mel is the log of the
    `lin` of the same call to within one float32 ulp - the bin <-> register <-> lane-half map of the accumulator-as-B product and the Nyquist
    step, with no tolerance to hide in."""
    n_fft, hop, win = 256, 64, 256
    over, wav = EH.mel_signal(flavour, n_fft, hop, 65)
    name, o = flavour, EH.flavour_options(flavour, over, n_fft, hop)
    for basis, shift in EH.onehot_bases(n_fft):
        got, lin = ST.logmel_op(wav.to(DEV), torch.from_numpy(basis).to(DEV), n_fft=n_fft, hop=hop, win_length=win, flavour=flavour, return_linear=True, **over)
        ulps = EH.onehot_ulps(got.cpu().numpy(), lin.cpu().numpy(), shift, o['floor'], o['log10'])
        print(f'logmel {name} one-hot rows on bins {shift} .. {shift + 127}: at most {ulps:.2f} float32 ulp from log(lin) of the same call (bound 1)')
        assert ulps <= 1


def test_lengths_outside_the_row():
    """lengths = [-5, 0, 1, L, L + 100] behaves as [0, 0, 1, L, L]: frame counts by the header formula, frames past the count exactly 0, valid
    rows bitwise their solo call - spectrum, log-mel and linear magnitude."""
    n_fft, hop, win, L = 512, 50, 240, 2000
    lens, eff = [-5, 0, 1, L, L + 100], [0, 0, 1, L, L]
    wav = SH.make_signal(L, seed=9, batch=5, noise=0.3).to(DEV)
    basis = torch.from_numpy(EH.dense_basis(33, n_fft)).to(DEV)
    T = 1 + L // hop
    counts = [EH.row_frames(n, n_fft, hop, n_fft // 2, n_fft // 2) for n in eff]
    assert counts == [0, 0, 1, T, T]
    spec, fc = ST.stft_op(wav, n_fft=n_fft, hop=hop, win_length=win, lengths=torch.tensor(lens), return_frames=True)
    mel, lin, fc2 = ST.logmel_op(wav, basis, n_fft=n_fft, hop=hop, win_length=win, flavour='pwg', lengths=torch.tensor(lens), return_linear=True, return_frames=True)
    assert spec.shape == (5, n_fft // 2 + 1, T) and mel.shape == (5, T, 33) and lin.shape == (5, T, n_fft // 2 + 1)
    assert fc.cpu().tolist() == counts and fc2.cpu().tolist() == counts
    for b, n in enumerate(eff):
        t = counts[b]
        assert not bool(torch.view_as_real(spec[b, :, t:]).any()) and not bool(mel[b, t:].any()) and not bool(lin[b, t:].any())
        if n:
            solo = ST.stft_op(wav[b:b + 1, :n], n_fft=n_fft, hop=hop, win_length=win)
            smel, slin = ST.logmel_op(wav[b:b + 1, :n], basis, n_fft=n_fft, hop=hop, win_length=win, flavour='pwg', return_linear=True)
            assert _bits(solo[0], spec[b, :, :t]) and torch.equal(smel[0], mel[b, :t]) and torch.equal(slin[0], lin[b, :t]), b
    print(f'lengths {lens} on L={L}: frame counts {counts}, frames past the count exactly 0, valid rows bitwise their solo call (spectrum, log-mel, magnitude)')


def test_reflect_rows_no_longer_than_their_padding():
    """include/dsv.h, `lengths`: in reflect mode a row no longer than its padding is padded by ONE reflection about its own first / last sample
    and 0 where that leaves the row (the host checks L, not lengths[b])."""
    n_fft, hop, win = 512, 128, 512
    c = EH.ragged_reflect_case(n_fft, hop, win)
    got, fc = ST.stft_op(c['wav'].to(DEV), n_fft=n_fft, hop=hop, win_length=win, pad_mode='reflect', lengths=torch.tensor(c['lens']), return_frames=True)
    assert got.shape[2] == c['T'] and fc.cpu().tolist() == [1 + n // hop for n in c['lens']]
    for b, (n, want) in enumerate(zip(c['lens'], c['refs'])):
        t = int(fc[b])
        assert not bool(torch.view_as_real(got[b, :, t:]).any())
        err = EH.cerr(got[b:b + 1, :, :t], want)
        tight = c['tight'][b]
        bound, why = (2 * c['yard'], '2 x the yardstick of the whole batch') if tight is None else (tight, '(n + 1) u sum |x|: a sum of n <= 2 products')
        print(f'reflect row of {n} sample(s), padding {n_fft // 2} ({t} frames): max-abs err {err:.3e}, bound {bound:.3e} ({why})')
        assert err <= bound, (n, err, bound)
