"""CPU: the case tables of tests/fs2_loss_edge_helpers.py hold the tiles, seams and limits of the FastSpeech2 training objective
(csrc/fs2_loss.hpp) they claim to hold, the float64 references of tests/test_gpu_fs2_loss_edges.py run on every row of them, and the yardstick
catches the faults the shapes exist for.

  * kMlTile, kMlMaxM, kDurMaxTxt and the 256-thread block widths are the header's (parsed from its text) and losses.py's limits;
  * TABLE MEL holds every frame count one short of, at and one past one and two tiles, the counts at which the 5- and 10-frame halo first fits
    or reaches the next tile, a case of three tiles, 255 / 256 / 257 partial sums, M = 1, 5, 10, 11, 12, 127 and kMlMaxM, bias 20 on the
    11-wide view, every stride layout, and every zero-frame pattern at T = 33 and 48 with a prediction left on the emptied frames;
  * TABLE DUR holds T_txt = 1 .. kDurMaxTxt on both sides of every chunk size, words that straddle every chunk seam, slot T_txt - 1, the
    silence placements, empty rows, the clamp's edge, word_boundary = 2 inside and past the word buffer;
  * every reference runs once, is finite, and counts weighted frames, phones and kept words;
  * six restated faults - SSIM per tile with a zero halo, a backward halo of 5, the row weight of the neighbouring frame, a prefix scan without
    its chunk offsets, a word sum cut at a chunk seam, clamp's backward as > 0 - exceed the allowance at a table case, and the unfaulted
    restatement of each stays inside it."""
import pytest
import torch
import torch.nn.functional as F

from tests import fs2_loss_edge_helpers as V
from tests import fs2_loss_helpers as LH

MEL, DUR = V.mel_cases(), V.dur_cases()
F64, F32 = torch.float64, torch.float32


def test_constants_are_the_headers():
    from diffsinger_amd import losses
    assert (V.TILE, V.MAX_M, V.MAX_TXT) == (16, losses.MAX_BINS, losses.MAX_PHONES) == (16, 128, 2048)
    assert V.BLOCK == V.FINAL_BLOCK == 256 and all(V.launch_bounds(k) == 256 for k in ('k_mel_loss_fwd', 'k_mel_loss_bwd'))
    assert V.WINDOW == 11 and V.HALO == 5
    assert len(set(MEL)) == len(MEL) and len(set(DUR)) == len(DUR)


def test_mel_table_holds_the_tiles_seams_and_limits():
    t, h = V.TILE, V.HALO
    sweep = {c.T for c in MEL if c.M == 80 and c.bias == 6.0 and c.zero == 'tail'}
    named = {1, h, h + 1, 2 * h, 2 * h + 1, t - 1, t, t + 1, t + h, t + 2 * h, t + 2 * h + 1, 2 * t - 1, 2 * t, 2 * t + 1, 3 * t}
    assert named <= sweep and {T % t for T in named} <= {T % t for T in sweep}
    assert any(T < V.WINDOW for T in sweep) and any(V.tiles(c.T) >= 3 for c in MEL)
    assert {c.M for c in MEL if c.T == 2 * t + 1 and c.bias == 6.0} >= {1, h, 2 * h, V.WINDOW, V.WINDOW + 1, V.MAX_M - 1, V.MAX_M}
    assert any(c.M == 10 and c.bias == 20.0 and c.layout == 'cwt' for c in MEL)
    assert {c.B * V.tiles(c.T) for c in MEL} >= {V.FINAL_BLOCK - 1, V.FINAL_BLOCK, V.FINAL_BLOCK + 1}
    assert {c.B for c in MEL} == {1, 3}
    assert {c.layout for c in MEL} == set(V.LAYOUTS) | {'mixed_rev'}
    for T in V.ZERO_T:
        assert {c.zero for c in MEL if c.T == T} >= set(V.ZERO_PATTERNS)
    assert [V.zero_frames(z, 33) for z in ('z15', 'z16', 'z15_16', 'zlast')] == [[t - 1], [t], [t - 1, t], [32]]
    for z in ('run10_21', 'run6_27'):                                           # both runs cross the seam; the long one by more than 2 * halo a side
        fr = V.zero_frames(z, 48)
        assert fr[0] < t <= fr[-1] and fr == list(range(fr[0], fr[-1] + 1))
    fr = V.zero_frames('run6_27', 48)
    assert t - fr[0] >= 2 * h and fr[-1] + 1 - t > 2 * h


def test_mel_operands_are_what_the_patterns_say():
    for c in MEL:
        x, y = V.mel_operands(c)
        w = V.mel_weights(y)[:, :, 0]
        assert x.shape == y.shape == (c.B, c.T, c.M) and float(w.sum()) > 0
        fr = V.zero_frames(c.zero, c.T)
        if c.zero == 'lastbin':
            assert bool((w[:, 16] == 1).all()) and bool((y[:, 16, :-1] == 0).all()) and bool((w[:, [15, 17]] == 0).all())
            fr = [15, 17]
        if c.zero == 'negzero':
            assert bool(torch.signbit(y[:, fr]).all())
        if c.zero == 'utt':
            assert float(w[c.B - 1].sum()) == 0 and float(w[0].sum()) > 0 and float(x[c.B - 1].abs().min()) > 0
        if fr:
            assert bool((w[:, fr] == 0).all()) and float(x[c.B - 1, fr].abs().min()) > 0     # a prediction on frames the weights must drop


def test_every_mel_reference_runs_and_is_finite():
    for c in MEL:
        r = V.mel_case_reference(c, F64)
        assert bool(torch.isfinite(r['out']).all()) and bool(torch.isfinite(r['map']).all()) and bool(torch.isfinite(r['dx']).all()), V.mel_id(c)
        assert float(r['out'][3]) > 0 and float(r['out'][3]) % c.M == 0 and float(r['dx'].abs().max()) > 0
        assert r['map'].shape == r['dx'].shape == (c.B, c.T, c.M)
    # the cross of the GPU test: every combination the ABI admits runs under autograd
    c = V.MelCase(3, 33, 80, 6.0, 'tail', 'contig')
    x, y = V.mel_operands(c)
    for terms in (1, 2, 3):
        for weighted in (0, 1):
            for R in ((None, V.mel_grad_map(c)) if terms & 2 else (None,)):
                r = V.mel_reference(x, y, 6.0, terms, weighted, (0.7, 1.3), (0.9, 1.1, 0.4), R)
                assert bool(torch.isfinite(r['dx']).all()) and float(r['out'][3]) == (V.mel_weights(y).sum() if weighted else y.numel())
                assert (r['map'] is None) == (not terms & 2)


def test_dur_table_holds_the_chunks_seams_and_limits():
    tts = {c.Tt for c in DUR}
    assert tts >= {1, 2, V.BLOCK - 1, V.BLOCK, V.BLOCK + 1, 2 * V.BLOCK - 1, 2 * V.BLOCK, 2 * V.BLOCK + 1, V.MAX_TXT - 1, V.MAX_TXT}
    for Tt in V.DUR_TT:
        assert {c.seg for c in DUR if c.Tt == Tt} == set(V.SEGS)
    assert {c.T for c in DUR if c.Tt == 12} >= {1, V.BLOCK - 1, V.BLOCK, V.BLOCK + 1}
    assert {c.B for c in DUR} == {1, 3}
    assert all(abs(c.T - 3 * c.Tt) <= 2 for c in DUR if c.Tt != 12)
    straddle = [c for c in DUR if c.pat == 'straddle']
    assert {V.chunk_of(c.Tt) for c in straddle} >= {2, 3, 8} and {c.seg for c in straddle} == set(V.SEGS)
    for c in straddle:                                                          # every chunk seam lies inside a kept word
        s, k = V.word_slots(V.dur_operands(c)), V.chunk_of(c.Tt)
        seams = torch.arange(k, c.Tt, k)
        assert len(seams) and bool((s[:, seams] == s[:, seams - 1]).all()) and bool((s[:, seams] >= 0).all()), V.dur_id(c)


def test_dur_operands_are_what_the_patterns_say():
    seen = set()
    for c in DUR:
        o, f = V.dur_operands(c), V.dur_flags(c)
        tok, m2p, s, Tt = o['tok'], o['mel2ph'], V.word_slots(o), c.Tt
        assert int(m2p.min()) >= 0 and int(m2p.max()) <= Tt and m2p.shape == (c.B, c.T)
        dur = LH.mel2ph_to_dur(m2p, Tt)
        phones, words = V.dur_counts(o)
        assert phones > 0 and (words > 0 or f['nan'] or f['no_word']), V.dur_id(c)
        sil = torch.zeros_like(tok).bool()
        for p in V.SIL:
            sil |= tok == p
        if c.pat == 'one_word':
            assert int(s.max()) == 0 and bool(((s == 0) | sil).all())
        if c.pat == 'all_ones':
            assert bool((s == torch.arange(Tt)).all()) and int(dur[:, Tt - 1].sum()) >= 0 and int(s.max()) == Tt - 1     # the buffer's last slot
        if c.pat == 'sil_edges':
            assert bool(sil[:, 0].all()) and bool(sil[:, Tt - 1].all()) and bool((sil[:, Tt // 3] & sil[:, Tt // 3 + 1]).all())
        if c.pat == 'row_nosil':
            assert not bool(sil[1].any()) and bool((s[1] < 0).all()) and bool(sil[0].any()) and bool(sil[2].any())
        if c.pat == 'pad_row':
            assert int(m2p[1].max()) == 0 and int(m2p[0].min()) > 0
        if c.pat == 'zero_frames':
            assert int(dur[:, [2, 6]].sum()) == 0
        if c.pat == 'long_phone':
            assert int(dur[0].max()) >= 3000
        if c.pat == 'dur_edge':
            d = o['dur_pred']
            assert bool((d[:, 1] == 0).all()) and bool((d[:, 2:4] < 0).all()) and bool((s[:, 1:4] >= 0).all())
        if c.pat == 'wdb_two':
            assert int(o['wdb'].max()) == 2 and int(s.max()) < Tt
        if c.pat == 'wdb_overflow':
            assert int(s.max()) == Tt and f['nan']
        if bool((tok[:, -1] == 0).any()) and bool((tok[0] > 0).all()):
            seen.add('padded phones')
        if bool((dur == 0)[tok > 0].any()):
            seen.add('phones without a frame')
        if bool((m2p[:, -1] == 0).any()):
            seen.add('padding frames')
        seen.add(c.pat)
    assert seen >= {'padded phones', 'phones without a frame', 'padding frames', 'random', 'straddle', 'one_word', 'all_ones', 'sil_edges', 'row_nosil',
                    'pad_row', 'zero_frames', 'long_phone', 'dur_edge', 'wdb_two', 'wdb_overflow'}
    assert any(c.pat == 'all_ones' and c.Tt == V.MAX_TXT for c in DUR) and any(c.pat == 'wdb_overflow' and c.Tt == V.MAX_TXT for c in DUR)


def test_every_dur_reference_runs_and_is_finite():
    for c in DUR:
        f = V.dur_flags(c)
        if f['nan']:
            continue
        r = V.dur_case_reference(c, F64)
        keep = [0, 2] if f['no_word'] else [0, 1, 2]
        assert bool(torch.isfinite(r['out'][keep]).all()) and bool(torch.isfinite(r['grad']).all()) and float(r['grad'].abs().max()) > 0, V.dur_id(c)


# ---- the yardstick catches the faults the shapes exist for ------------------------------------------------------------------------------
SEAM = V.MelCase(3, 33, 80, 6.0, 'tail', 'contig')
ONE_TILE = V.MelCase(3, 16, 80, 6.0, 'tail', 'mixed')


def _map_per_tile(c):
    """FAULT: the SSIM map of every 16-frame tile computed as an image of its own (zero halo)"""
    x, y = (t.double() for t in V.mel_operands(c))
    return torch.cat([LH.ssim_map(x[:, None, t0:t0 + V.TILE] + c.bias, y[:, None, t0:t0 + V.TILE] + c.bias).mean(1) for t0 in range(0, c.T, V.TILE)], 1)


def test_fault_ssim_per_tile_with_a_zero_halo():
    r64, r32 = V.mel_case_reference(SEAM, F64), V.mel_case_reference(SEAM, F32)
    ratio, row, e, allow = V.row_ratio(_map_per_tile(SEAM), r64['map'], r32['map'], V.FLOOR_MEL_VALUE)
    assert ratio > 100 and min(abs(row % SEAM.T - s) for s in (V.TILE, 2 * V.TILE)) <= V.HALO, (ratio, row)   # within the halo of a seam
    w = V.mel_weights(V.mel_operands(SEAM)[1]).double()
    wrong = float(((1 - _map_per_tile(SEAM)) * w).sum() / w.sum() * V.MEL_LAM[1])
    assert V.value_ratio(wrong, r64['out'][1], r32['out'][1], V.FLOOR_MEL_VALUE)[0] > 1
    one64, one32 = V.mel_case_reference(ONE_TILE, F64), V.mel_case_reference(ONE_TILE, F32)
    assert V.row_ratio(_map_per_tile(ONE_TILE), one64['map'], one32['map'], V.FLOOR_MEL_VALUE)[0] == 0       # one tile: the same thing


def _dx_with_halo(c, halo):
    """k_mel_loss_bwd's tiling restated: a tile's gradient from the frames [t0 - halo, t0 + 16 + halo) alone, dL/dS taken on the frames
    [t0 - 5, t0 + 21) the tile evaluates.  halo = 10 is the kernel; FAULT: halo = 5."""
    x, y = (t.double() for t in V.mel_operands(c))
    w = V.mel_weights(y)
    cmap = w * (V.MEL_GOUT[2] - V.MEL_LAM[1] * V.MEL_GOUT[1]) / w.sum() + V.mel_grad_map(c).double()
    l1 = V.MEL_GOUT[0] * V.MEL_LAM[0] * torch.sign(x - y) * w / w.sum()
    out = torch.zeros_like(x)
    for t0 in range(0, c.T, V.TILE):
        lo, hi = max(0, t0 - halo), min(c.T, t0 + V.TILE + halo)
        xc = x[:, lo:hi].clone().requires_grad_(True)
        keep = torch.zeros(hi - lo, 1, dtype=F64)
        keep[max(0, t0 - V.HALO) - lo:t0 + V.TILE + V.HALO - lo] = 1
        (LH.ssim_map(xc[:, None] + c.bias, y[:, None, lo:hi] + c.bias).mean(1) * cmap[:, lo:hi] * keep).sum().backward()
        out[:, t0:t0 + V.TILE] = xc.grad[:, t0 - lo:t0 - lo + V.TILE]
    return out + l1


def test_fault_backward_halo_of_five():
    r64, r32 = V.mel_case_reference(SEAM, F64), V.mel_case_reference(SEAM, F32)
    assert V.row_ratio(_dx_with_halo(SEAM, 2 * V.HALO), r64['dx'], r32['dx'], V.FLOOR_MEL_GRAD)[0] <= 1      # the kernel's halo: exact
    ratio, row, e, allow = V.row_ratio(_dx_with_halo(SEAM, V.HALO), r64['dx'], r32['dx'], V.FLOOR_MEL_GRAD)
    assert ratio > 100, (ratio, row)
    # ... and the per-tensor measure the per-row rule replaces: the same fault is far smaller on it
    whole = float((_dx_with_halo(SEAM, V.HALO) - r64['dx']).abs().max() / r64['dx'].abs().max())
    print(f'halo 5: per-row ratio {ratio:.0f} at row {row}, per-tensor relative error {whole:.1e}')
    one64, one32 = V.mel_case_reference(ONE_TILE, F64), V.mel_case_reference(ONE_TILE, F32)
    assert V.row_ratio(_dx_with_halo(ONE_TILE, V.HALO), one64['dx'], one32['dx'], V.FLOOR_MEL_GRAD)[0] <= 1  # one tile: nothing to cut


def test_fault_row_weight_of_the_neighbouring_frame():
    c = next(c for c in MEL if c.zero == 'z16' and c.T == 33)
    x, y = (t.double() for t in V.mel_operands(c))
    r64, r32 = V.mel_case_reference(c, F64), V.mel_case_reference(c, F32)
    w = torch.roll(V.mel_weights(y), 1, dims=1)                                  # FAULT: frame t weighted by frame t - 1's flag
    xr = x.clone().requires_grad_(True)
    smap = LH.ssim_map(xr[:, None] + c.bias, y[:, None] + c.bias).mean(1)
    o = [((xr - y).abs() * w).sum() / w.sum() * V.MEL_LAM[0], ((1 - smap) * w).sum() / w.sum() * V.MEL_LAM[1], (smap * w).sum() / w.sum()]
    (sum(g * v for g, v in zip(V.MEL_GOUT, o)) + (smap * V.mel_grad_map(c).double()).sum()).backward()
    assert float(w.sum()) == float(r64['out'][3])                               # the count cannot see it
    ratio, row, e, allow = V.row_ratio(xr.grad, r64['dx'], r32['dx'], V.FLOOR_MEL_GRAD)
    assert ratio > 100 and abs(row % c.T - V.TILE) <= V.HALO + 1, (ratio, row)
    assert V.value_ratio(o[0].detach(), r64['out'][0], r32['out'][0], V.FLOOR_MEL_VALUE)[0] > 1


STRADDLE = V.DurCase(3, 513, 1539, 'wdb', 'straddle')


def _wdur_by_slots(o, slots, dtype=F64):
    """fs2_loss_helpers.dur_loss's wdur with the word slots handed in"""
    d = o['dur_pred'].to(dtype)
    Tt = d.shape[1]
    gt = LH.mel2ph_to_dur(o['mel2ph'], Tt).to(dtype) * (o['tok'] != 0).to(dtype)
    lin = (d.exp() - 1).clamp(min=0)
    P = d.new_zeros(d.shape[0], Tt + 1).scatter_add(1, slots, lin)
    G = d.new_zeros(d.shape[0], Tt + 1).scatter_add(1, slots, gt)
    m = (G > 0).to(dtype)
    return (F.mse_loss((P + 1).log(), (G + 1).log(), reduction='none') * m).sum() / m.sum() * V.DUR_LAM['lam_word']


def test_fault_prefix_scan_without_its_chunk_offsets():
    assert STRADDLE in DUR
    o, k = V.dur_operands(STRADDLE), V.chunk_of(STRADDLE.Tt)
    r64, r32 = V.dur_case_reference(STRADDLE, F64), V.dur_case_reference(STRADDLE, F32)
    assert V.value_ratio(_wdur_by_slots(o, V.word_slots(o)), r64['out'][1], r32['out'][1], V.FLOOR_DUR, 1e-3)[0] <= 1
    wdb = o['wdb']
    pad = (-STRADDLE.Tt) % k
    cs = F.pad(wdb, (0, pad)).view(wdb.shape[0], -1, k).cumsum(-1).view(wdb.shape[0], -1)[:, :STRADDLE.Tt]   # FAULT: every chunk counts from 0
    assert k == 3 and int((cs - wdb).max()) < k
    assert V.value_ratio(_wdur_by_slots(o, cs - wdb), r64['out'][1], r32['out'][1], V.FLOOR_DUR, 1e-3)[0] > 100


def test_fault_word_sum_cut_at_a_chunk_seam():
    o, k = V.dur_operands(STRADDLE), V.chunk_of(STRADDLE.Tt)
    r64, r32 = V.dur_case_reference(STRADDLE, F64), V.dur_case_reference(STRADDLE, F32)
    cut = dict(o, wdb=o['wdb'].clone())
    cut['wdb'][:, torch.arange(k, STRADDLE.Tt, k) - 1] = 1                      # FAULT: a word ends where a thread's chunk ends
    got = V.dur_reference(cut, V.dur_gout(STRADDLE))
    assert V.value_ratio(got['out'][1], r64['out'][1], r32['out'][1], V.FLOOR_DUR, 1e-3)[0] > 100
    assert V.row_ratio(got['grad'], r64['grad'], r32['grad'], V.FLOOR_DUR)[0] > 100
    assert float(got['out'][0]) == float(r64['out'][0]) and float(got['out'][2]) == float(r64['out'][2])    # pdur and sdur cannot see it


@pytest.mark.parametrize('seg', V.SEGS)
def test_fault_clamp_backward_as_greater_than_zero(seg):
    c = V.DurCase(3, 12, 36, seg, 'dur_edge')
    assert c in DUR
    o, g = V.dur_operands(c), V.dur_gout(c)
    r64, r32 = V.dur_case_reference(c, F64), V.dur_case_reference(c, F32)
    only_p = V.dur_reference(o, [g[0], 0.0, 0.0])['grad']                        # FAULT: at dur_pred == 0 nothing flows through the clamp
    wrong = torch.where(o['dur_pred'] == 0, only_p, r64['grad'])
    assert int((o['dur_pred'] == 0).sum()) == c.B + 1 and not torch.equal(wrong, r64['grad'])
    assert V.row_ratio(wrong, r64['grad'], r32['grad'], V.FLOOR_DUR)[0] > 100
    below = o['dur_pred'] < 0                                                   # below the edge the clamp passes nothing: only pdur's gradient
    assert bool(below.any()) and torch.equal(r64['grad'][below], only_p[below])
