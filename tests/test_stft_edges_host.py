"""CPU: the edge cases of tests/test_gpu_stft_edges.py replayed without a device (tests/stft_edge_helpers.py).
  - the float64 inverse restatement against torch.istft wherever torch accepts the input, the inverse yardstick basis against numpy's irfft;
  - the unmutated float32 restatements of the kernels' index arithmetic stay inside every bound at every listed case: the bounds are
    satisfiable by the reference alone;
  - every restated bug (a) - (g) exceeds the bound of at least one listed case; the factor is printed, and whether the shapes of
    tests/test_gpu_stft.py would have seen it.
No GPU: nothing here launches a kernel."""
import numpy as np
import pytest
import torch

from tests import stft_edge_helpers as EH
from tests import stft_helpers as SH


def test_plan_restatement_has_the_forms_the_cases_are_chosen_for():
    assert EH.plan(2048, 300) == (256, 256)                  # chunked, KC < hop
    assert EH.plan(2048, 240) == (2048, 240) and EH.plan(1024, 120) == (1024, 120) and EH.plan(512, 50) == (512, 50)
    assert EH.plan(256, 75) == (256, 75) and EH.plan(256, 1) == (256, 1) and EH.plan(256, 256) == (256, 256)
    assert EH.plan(2048, 512) == (256, 256) and EH.plan(1024, 256) == (1024, 256)
    for n_fft in (512, 1024, 2048):
        assert EH.plan(n_fft, n_fft) == (256, 256)           # the inverse (frame stride n_fft) runs in chunks
    for n_fft, hop, _ in EH.FORWARD_GEOMS + EH.OLD_GEOMS:
        KC, RL = EH.plan(n_fft, hop)
        assert (EH.NF_WG - 1 + (KC + RL - 1) // RL) * (RL + 2) * 4 <= EH.LDS_BUDGET and n_fft % KC == 0
    # the cross-wave mel sum needs more LDS than the staged window (`red > lds` in dsv_logmel): at 512/50 from M = 33 on, at 256/64 from M = 80
    # on; M = 1 stays below at both, so both sides of the branch are run
    taken = {}
    for n_fft, hop, _ in EH.MEL_GEOMS:
        KC, RL = EH.plan(n_fft, hop)
        lds = (EH.NF_WG - 1 + (KC + RL - 1) // RL) * (RL + 2) * 4
        taken[(n_fft, hop)] = [M for M in EH.MEL_ROWS if EH.NF_WG * ((M + 31) // 32 * 32 + 1) * 4 > lds]
    assert taken == {(256, 64): [80, 128], (512, 50): [33, 80, 128]}, taken


def test_zsplit_restatement_and_where_a_workgroup_loops_over_row_groups():
    """A workgroup loops over more than one row group only where grid.z < ngroups.  n_fft = 256 has one group: its launches are never split and
    never loop.  Every other spectrum / inverse case of tests/test_gpu_stft.py and of the forward and inverse lists here has fewer than 512
    workgroups and is split into one group per z; only the unsplit cases with n_fft >= 512 run the loop."""
    assert [EH.row_groups(n) for n in (256, 512, 1024, 2048)] == [1, 2, 4, 8]
    for n_fft, hop, win, B, T in EH.UNSPLIT_CASES + [EH.UNSPLIT_INVERSE]:
        assert (T + 63) // 64 * B >= 512 and EH.zsplit(T, B, n_fft) == 1
        if n_fft == 256:
            assert EH.row_groups(n_fft) == 1 and EH.zsplit(T, 1, n_fft) == 1          # the B = 1 call is the same plan: one group, no split
        else:
            assert EH.row_groups(n_fft) > 1 and EH.zsplit(T, 1, n_fft) == EH.row_groups(n_fft)   # the B = 1 call: one group per z, no loop
    assert EH.plan(512, 128)[0] == 512 and EH.plan(2048, 300)[0] == 256 and EH.plan(512, 512)[0] == 256   # window reused / re-staged per group
    calls = [(g[0], max(c[0] for c in EH.forward_cases(*g)), EH.ROWS) for g in EH.FORWARD_GEOMS]      # (n_fft, most frames, rows)
    calls += [(g[0], max(EH.INVERSE_FRAMES), EH.ROWS) for g in EH.INVERSE_GEOMS] + [(g[0], 67, EH.ROWS) for g in EH.SUBTRACT_GEOMS]
    calls += [(g[0], 1 + 24000 // g[1], 1) for g in EH.OLD_GEOMS] + [(1024, 1025, 8), (512, 71, 4)]    # tests/test_gpu_stft.py: its largest calls
    for n_fft, T, B in calls:
        assert EH.zsplit(T, B, n_fft) == EH.row_groups(n_fft), (n_fft, T, B)


def test_float64_inverse_is_torch_istft_where_torch_accepts():
    accepted = []
    for n_fft, hop, win in EH.INVERSE_GEOMS:
        dirty, clean = EH.inverse_case(n_fft, hop, win, 65, rows=2)
        for center in (True, False):
            try:
                want = torch.istft(clean.to(torch.complex128), n_fft, hop_length=hop, win_length=n_fft, window=SH.window64(n_fft, win), center=center)
            except RuntimeError:
                continue
            got = EH.ref_istft_ola64(dirty, n_fft, hop, win, center)[0]
            assert got.shape == tuple(want.shape)
            err = float(np.abs(got - want.numpy()).max())
            accepted.append((n_fft, hop, win, center))
            print(f'ref_istft_ola64 {n_fft}/{hop}/{win} center={int(center)}: max-abs vs torch.istft {err:.2e} (bound 1e-12)')
            assert err <= 1e-12
    assert all(g + (True,) in accepted for g in [(512, 128, 512), (1024, 256, 800), (2048, 240, 1200)]), accepted
    assert not any(a[:3] == (1024, 256, 200) for a in accepted)            # gaps in the window sum: torch refuses, the operator does not


def test_inverse_yardstick_basis_is_irfft():
    for n_fft, hop, win in EH.INVERSE_GEOMS:
        g = torch.Generator().manual_seed(n_fft)
        S = torch.complex(torch.randn(2, n_fft // 2 + 1, 3, generator=g, dtype=torch.float64), torch.randn(2, n_fft // 2 + 1, 3, generator=g, dtype=torch.float64))
        fr = torch.matmul(EH.spectrum_rows(S), torch.from_numpy(EH.inverse_basis64(n_fft, win)).t()).numpy()
        X = S.numpy().transpose(0, 2, 1).copy()
        X[..., 0] = X[..., 0].real
        X[..., -1] = X[..., -1].real
        want = np.fft.irfft(X, n=n_fft, axis=-1) * SH.window64(n_fft, win).numpy()
        assert float(np.abs(fr - want).max()) <= 1e-12


def _report(name, text, factors, old=None):
    worst = max(factors.values()) if factors else 0.0
    where = max(factors, key=factors.get) if factors else None
    seen = '' if old is None else f'; at the shapes of tests/test_gpu_stft.py: {"visible" if old > 1 else "NOT visible"} ({old:.3g} x)'
    print(f'mutant ({name}) {text}: exceeds its bound in {sum(v > 1 for v in factors.values())} of {len(factors)} cases, at most {worst:.3g} x the bound at {where}{seen}')
    assert worst > 1, f'mutant ({name}) is caught by no listed case'


@pytest.mark.parametrize('n_fft,hop,win', EH.FORWARD_GEOMS)
def test_forward_restatement_inside_every_bound(n_fft, hop, win):
    worst = 0.0
    for T, L, center, mode in EH.forward_cases(n_fft, hop, win):
        c = EH.forward_case(n_fft, hop, win, T, L, center, mode)
        got, _ = EH.restate_stft32(c['wav'], n_fft, hop, win, center, mode)
        share = EH.cerr(got, c['want']) / (2 * c['yard'])
        worst = max(worst, share)
        assert share <= 1, (n_fft, hop, win, T, L, center, mode, share)
    print(f'forward restatement {n_fft}/{hop}/{win}, unmutated: at most {worst:.2f} of the bound over its cases')


def test_staging_mutants_outside():
    """Each mutant over ALL listed cases of the smallest geometries at which its switch changes anything ((a): frame 63 exists; (b): RL odd;
    (g): more than one chunk - of the listed geometries only 2048/300)."""
    fact = {m: {} for m in 'abg'}
    where = {'a': [(256, 75, 255), (256, 256, 256)], 'b': [(256, 75, 255), (256, 1, 256)], 'g': [(2048, 300, 1200)]}
    for n_fft, hop, win in EH.FORWARD_GEOMS:
        KC, RL = EH.plan(n_fft, hop)
        assert (RL % 2 == 1) == ((n_fft, hop, win) in where['b']) and (KC < n_fft) == ((n_fft, hop, win) in where['g'])
        ms = [m for m in 'abg' if (n_fft, hop, win) in where[m]]
        for T, L, center, mode in EH.forward_cases(n_fft, hop, win) if ms else []:
            c = EH.forward_case(n_fft, hop, win, T, L, center, mode)
            for m in ms:
                if m == 'a' and T < EH.NF_WG:
                    continue                                                 # the switch changes nothing here
                bad, _ = EH.restate_stft32(c['wav'], n_fft, hop, win, center, mode, mutant=m)
                fact[m][(n_fft, hop, win, T, L, int(center), mode)] = EH.cerr(bad, c['want']) / (2 * c['yard'])
    old = {m: 0.0 for m in 'abg'}
    for n_fft, hop, win in EH.OLD_GEOMS:
        for T, L, center, mode in EH.old_forward_cases(n_fft, hop, win):
            c = EH.forward_case(n_fft, hop, win, T, L, center, mode, rows=1)
            for m in 'abg':
                bad, _ = EH.restate_stft32(c['wav'], n_fft, hop, win, center, mode, mutant=m)
                old[m] = max(old[m], EH.cerr(bad, c['want']) / (2 * c['yard']))
    _report('a', 'seam: last frame of a workgroup one hop late', fact['a'], old['a'])
    _report('b', 'row wrap one sample short at odd RL', fact['b'], old['b'])
    _report('g', 'later KC chunks staged from n0 = 0', fact['g'], old['g'])
    assert old['b'] <= 1                                                     # every hop of the old shapes is even: (b) is visible only here


def test_inverse_restatement_inside_and_gather_mutants_outside():
    fact = {m: {} for m in 'ef'}
    w_fr = w_out = 0.0
    for n_fft, hop, win in EH.INVERSE_GEOMS:
        for T in EH.INVERSE_FRAMES:
            dirty, clean = EH.inverse_case(n_fft, hop, win, T)
            for center in (True, False):
                for length, fc in EH.inverse_calls(n_fft, hop, T, center):
                    ref = EH.inverse_refs(dirty, n_fft, hop, win, center, length, fc)
                    Y = ref['Y']
                    fr = EH.inverse_yardstick32(dirty, n_fft, win, fc).numpy()
                    out = EH.restate_ola32(fr, n_fft, hop, win, center, length, fc)
                    e_fr, share, bad = EH.judge_inverse(ref, fr, out)
                    assert e_fr <= 2 * Y and share <= 1 and bad == 0, (n_fft, hop, win, T, center, length, fc, e_fr, Y, share, bad)
                    w_fr, w_out = max(w_fr, e_fr / (2 * Y)), max(w_out, share)
                    for m in 'ef':
                        if m == 'f' and fc is None:
                            continue
                        o = EH.restate_ola32(fr, n_fft, hop, win, center, length, fc, mutant=m)
                        _, s, b = EH.judge_inverse(ref, fr, o)
                        fact[m][(n_fft, hop, win, T, int(center), length, fc is not None)] = float('inf') if b else s
    print(f'inverse restatement, unmutated: frames at most {w_fr:.2f} of 2 Y, output at most {w_out:.2f} of the per-sample bound')
    _report('e', 'overlap-add without the last contributing frame', fact['e'])
    _report('f', 'window sum over all frames instead of frame_counts', fact['f'])


def test_subtraction_restatement_inside():
    for n_fft, hop, win in EH.SUBTRACT_GEOMS:
        c = EH.subtract_case(n_fft, hop, win)
        S32 = SH.yardstick32(c['wav'], n_fft, hop, win)
        for v in c['vs']:
            share, bad = EH.judge_subtract(EH.soft_threshold32(S32, v), c, v)
            print(f'subtraction restatement {n_fft}/{hop}/{win} v={v:.4g}: {share:.2f} of the element-wise bound, {bad} element(s) not exactly 0 that must be')
            assert share <= 1 and bad == 0
        assert not bool(torch.view_as_real(EH.soft_threshold32(S32, c['vs'][-1])).any())


def test_mel_restatement_inside_and_nyquist_mutant_outside():
    fact = {}
    worst = 0.0
    for n_fft, hop, win in EH.MEL_GEOMS:
        for flavour in ('pwg', 'hifigan'):
            for T in (65, 1):
                over, wav = EH.mel_signal(flavour, n_fft, hop, T)
                for M in EH.MEL_ROWS:
                    basis = EH.dense_basis(M, n_fft)
                    r = EH.logmel_refs(wav, basis, flavour, over, n_fft, hop, win)
                    want, yard = r['want'], r['yard']
                    assert want.shape[1] == T and float(r['mel'].min()) >= 1e-3, (want.shape, float(r['mel'].min()))
                    got, _ = EH.restate_logmel32(wav, basis, flavour, n_fft, hop, win, over=over)
                    share = float((got.double() - want).abs().max()) / (2 * yard)
                    worst = max(worst, share)
                    assert share <= 1, (n_fft, hop, flavour, T, M, share)
                    bad, _ = EH.restate_logmel32(wav, basis, flavour, n_fft, hop, win, mutant='c', over=over)
                    fact[('dense', n_fft, hop, flavour, T, M)] = float((bad.double() - want).abs().max()) / (2 * yard)
    print(f'dense-basis mel restatement, unmutated: at most {worst:.2f} of the bound')
    n_fft, hop, win = 256, 64, 256
    for flavour in ('pwg', 'hifigan'):
        over, wav = EH.mel_signal(flavour, n_fft, hop, 65)
        o = EH.flavour_options(flavour, over, n_fft, hop)
        for basis, shift in EH.onehot_bases():
            got, lin = EH.restate_logmel32(wav, basis, flavour, n_fft, hop, win, over=over)
            assert EH.onehot_ulps(got.numpy(), lin.numpy(), shift, o['floor'], o['log10']) <= 1
            bad, lin = EH.restate_logmel32(wav, basis, flavour, n_fft, hop, win, mutant='c', over=over)
            fact[('one-hot', flavour, shift)] = EH.onehot_ulps(bad.numpy(), lin.numpy(), shift, o['floor'], o['log10'])
    # the old shapes (tests/test_gpu_stft.py::test_logmel_against_float64) replayed with the shipped filterbanks: fmin > 0 and fmax < sr / 2 weigh
    # bin 0 and the Nyquist bin with exactly 0, so the mutant's mel is the unmutated mel, bit for bit
    from diffsinger_amd.stft import mel_filterbank
    old = 0.0
    for (n_fft, hop), (sr, M, fmin, fmax) in (((512, 128), (24000, 80, 50, 11025)), ((1024, 256), (22050, 80, 80, 7600))):
        basis = mel_filterbank(sr, n_fft, M, fmin, fmax)
        assert not basis[:, [0, -1]].any()
        for flavour in ('pwg', 'hifigan'):
            wav = SH.make_signal(9000, seed=9000 + n_fft, batch=1, noise=0.3) * (1.3 if flavour == 'hifigan' else 1.0)
            r = EH.logmel_refs(wav, basis, flavour, None, n_fft, hop, n_fft)
            good, _ = EH.restate_logmel32(wav, basis, flavour, n_fft, hop, n_fft)
            bad, _ = EH.restate_logmel32(wav, basis, flavour, n_fft, hop, n_fft, mutant='c')
            assert torch.equal(good, bad)
            old = max(old, float((bad.double() - r['want']).abs().max()) / (2 * r['yard']))
    _report('c', 'Nyquist weight left out of the mel (dense: x the bound; one-hot: ulps against 1)', fact, old)


def test_ragged_reflect_restatement_inside_and_reflection_mutant_outside():
    c = EH.ragged_reflect_case()
    n_fft, hop, win = 512, 128, 512
    got, counts = EH.restate_stft32(c['wav'], n_fft, hop, win, True, 'reflect', lengths=c['lens'])
    bad, _ = EH.restate_stft32(c['wav'], n_fft, hop, win, True, 'reflect', lengths=c['lens'], mutant='d')
    assert counts == [1 + n // hop for n in c['lens']]
    fact = {}
    yard = c['yard']
    for b, (n, want) in enumerate(zip(c['lens'], c['refs'])):
        t = counts[b]
        assert want.shape[2] == t and not bool(torch.view_as_real(got[b, :, t:]).any())
        bound = 2 * yard if c['tight'][b] is None else c['tight'][b]           # rows of one or two samples: their own rounding condition
        share = EH.cerr(got[b:b + 1, :, :t], want) / bound
        assert share <= 1, (n, share)
        fact[(n_fft, hop, 'len', n)] = EH.cerr(bad[b:b + 1, :, :t], want) / bound
    # the old ragged batch (tests/test_gpu_stft.py::test_forward_ragged_batch, reflect): rows longer than their padding
    wav = SH.make_signal(9000, seed=3, batch=4)
    lens = [9000, 5000, 700, 0]
    bad, _ = EH.restate_stft32(wav, n_fft, hop, win, True, 'reflect', lengths=lens, mutant='d')
    old = 0.0
    for b, n in enumerate(lens[:3]):
        want = SH.ref_stft64(wav[b, :n], n_fft, hop, win, True, 'reflect')
        yard = EH.cerr(SH.yardstick32(wav[b, :n], n_fft, hop, win, True, 'reflect'), want)
        old = max(old, EH.cerr(bad[b:b + 1, :, :want.shape[2]], want) / (2 * yard))
    _report('d', 'a ragged row reflects about L instead of its own end', fact, old)


def test_lengths_outside_the_row_clamp_in_the_restatement():
    n_fft, hop, win, L = 512, 128, 512, 2000
    wav = SH.make_signal(L, seed=5, batch=5)
    got, counts = EH.restate_stft32(wav, n_fft, hop, win, lengths=[-5, 0, 1, L, L + 100])
    assert counts == [0, 0, 1, 1 + L // hop, 1 + L // hop]
    full, _ = EH.restate_stft32(wav[3:], n_fft, hop, win)
    assert torch.equal(torch.view_as_real(got[3:]), torch.view_as_real(full)) and not bool(torch.view_as_real(got[:2]).any())
