"""CPU: the case tables of tests/voc_train_edge_helpers.py hold the paths of the vocoder's training kernels they claim to hold, and the float64
references of tests/test_gpu_voc_train_edges.py run on every row of them.

  * the slab and span constants behind the dispatch restatement are csrc/voc_kernels.hpp's (kVocHalo, kVocHaloWide, kVocLdsBudget parsed from the
    header text), the split and chunk lengths csrc/voc_train_common.hpp's and csrc/hifigan_train.hpp's;
  * TABLE DGRAD reaches all four builds of k_hgt_dgrad; per build a one-slab case, a second slab that is a multiple of 8 and one that is not; three
    slabs; a clamped wave on both <2,2> builds; a partial row block above 32 rows; both one-sided wide cases; each wide build at reach 36 and 48;
    every instantiation at L = 1, SPAN - 1, SPAN, SPAN + 1, the wide ones at 35, 47, 48, 49, in `second` form and without a mask;
  * the other tables hold 8, 12 and 15 splits, 256, 257 and 270 row-sum partials, a transposed case with more than one split, 192 polyphase
    rows, aux 40, 64, 72, 128, noise strides 6 and 15 and L_out = 1 and 2;
  * every reference runs once on seeded float32 operands: shapes as the device lays them out, and a bound that is non-zero wherever the GPU test
    expects a non-zero result (a zero bound there would demand exact zeros of a correct kernel);
  * three restated bugs - a dropped remainder slab, a split reduction that stops after 8 splits, a row sum that makes one pass over its partials -
    exceed the bound wherever the tables can see them and are the exact result everywhere else;
  * the module configurations of the GPU test reach the wide builds they are for."""
import pytest
import torch

from tests import hifigan_train_helpers as TH
from tests import pwg_train_helpers as PH
from tests import voc_edge_helpers as E
from tests import voc_train_edge_helpers as V

S = V.header_constant('voc_train_common.hpp', 'kSplitK')


def test_constants_are_the_headers():
    halo, wide, budget = (V.header_constant('voc_kernels.hpp', n) for n in ('kVocHalo', 'kVocHaloWide', 'kVocLdsBudget'))
    assert (halo, wide, budget) == (E.HALO, E.HALO_WIDE, E.LDS_BUDGET) == (28, 48, 72 * 1024)
    for tag, (nb, wt, h) in V.BUILDS.items():
        assert h == (wide if tag.endswith('wide') else halo)
        assert E.slab_of(nb, wt, h) == E.SLABS[tag] == min(256, budget // ((32 * nb * wt + 2 * h) * 4) // 8 * 8)
        assert E.span_of(nb, wt) == E.SPANS[tag]
    assert [E.SLABS[t] for t in ('<4,4>', '<2,2>', '<4,4>wide', '<2,2>wide')] == [32, 96, 24, 80]
    assert S == 512 and V.header_constant('hifigan_train.hpp', 'kHgtSumChunk') == V.SUM_CHUNK
    assert V.RULE is PH.RULE and V.U is PH.U and V.E_GATE is PH.E_GATE and V.RULE == TH.RULE


def test_taps_of_agrees_with_the_existing_test_and_the_product():
    from diffsinger_amd.hifigan_train import polyphase_taps
    from tests.test_gpu_hifigan_train import taps_of
    for u, k in sorted({(c[3], c[4]) for c in V.UP} | {(c[3], c[4]) for c in V.WGRAD_UP}):
        assert V.taps_of(k, u) == taps_of(k, u)
        r, t, kk, pad = polyphase_taps(k, u)
        assert (list(r), list(t), kk, pad) == tuple(V.taps_of(k, u))


def test_dgrad_table_reaches_every_path():
    rows = [(tag, V.dgrad_dispatch(C, Cg, K, dil, pad)) for tag, C, Cg, K, dil, pad in V.DGRAD]
    for tag, d in rows:
        assert d['tag'] == tag and d['span'] == E.SPANS[tag] and d['slab'] == E.SLABS[tag] and sum(d['slabs']) > 0
    assert {tag for tag, _ in rows} == set(V.BUILDS)
    for tag in V.BUILDS:
        mine = [d for t, d in rows if t == tag]
        assert any(len(d['slabs']) == 1 for d in mine), tag
        assert any(len(d['slabs']) > 1 and d['slabs'][-1] % 8 == 0 for d in mine), tag
        assert any(len(d['slabs']) > 1 and d['slabs'][-1] % 8 != 0 for d in mine), tag
    assert any(len(d['slabs']) == 3 for _, d in rows)
    assert any(len(d['slabs']) == 2 and t == '<4,4>wide' and sum(d['slabs']) == 32 for t, d in rows)          # the v3 32-channel stage: 24 + 8
    for tag in ('<2,2>', '<2,2>wide'):
        assert any(d['clamped'] and d['blocks'] % 2 == 1 for t, d in rows if t == tag), tag
    assert not any(d['clamped'] for t, d in rows if t.startswith('<4,4>'))
    assert any(C > 32 and C % 32 != 0 for _, C, *_ in V.DGRAD)
    assert any(d['z'] == 4 for _, d in rows)
    assert {d['wide_by'] for _, d in rows} >= {(False, True), (True, False), (True, True), (False, False)}
    for tag in ('<4,4>wide', '<2,2>wide'):
        assert {36, 48} <= {d['reach'] for t, d in rows if t == tag}
    assert any(pad != (K - 1) * dil - pad and not d['tag'].endswith('wide') for (_, _, _, K, dil, pad), (_, d) in zip(V.DGRAD, rows))


def test_dgrad_cases_hold_the_lengths_and_forms():
    cases = V.dgrad_cases()
    assert len(set(cases)) == len(cases) and V.DGRAD_REPEAT in cases
    for tag in V.BUILDS:
        span = E.SPANS[tag]
        first = next(r for r in V.DGRAD if r[0] == tag)
        mine = [c for c in cases if c[:6] == first]
        want = {1, span - 1, span, span + 1} | (set(V.WIDE_SHORT) if tag.endswith('wide') else set())
        assert {c[7] for c in mine if c[8] == 'first' and c[9]} == want
        assert any(c[8] == 'second' for c in mine) and any(not c[9] for c in mine)
        if tag.endswith('wide'):
            reach = V.dgrad_dispatch(*first[1:])['reach']
            assert min(V.WIDE_SHORT) < reach < max(V.WIDE_SHORT) or reach == 48
    for row in V.DGRAD:
        assert row + (2, E.SPANS[row[0]] + 1, 'first', True) in cases
    tag, C, Cg, K, dil, pad = V.DGRAD_REPEAT[:6]
    assert len(V.dgrad_dispatch(C, Cg, K, dil, pad)['slabs']) == 3


def test_the_other_tables_hold_what_they_claim():
    assert {V.splits_of(B, V.length(L, S), S) for B, _, _, _, L in V.WGRAD_PLAIN} == {8, 12, 15}
    assert V.splits_of(V.WGRAD_BITS[0], V.length(V.WGRAD_BITS[2], S), S) == 12
    assert any(u > 1 and V.splits_of(B, V.length(L, S), S) > B for B, _, _, u, _, L in V.WGRAD_UP)
    assert any(u > 1 and V.length(L, S) > 2 * S for _, _, _, u, _, L in V.WGRAD_UP)
    assert any(128 < Co * u < 256 for _, _, Co, u, _, _ in V.WGRAD_UP)
    assert {V.partials_of(B, L) for B, _, L in V.ROWSUM} >= {256, 257, 270}
    assert {L for _, _, L in V.ROWSUM} >= {1024, 1025}
    assert {(u, k) for _, _, _, u, k, _, _ in V.UP} == {(2, 2), (5, 11), (3, 7), (8, 16), (4, 8)}
    assert {L for *_, L, _ in V.UP} >= {1, 256, 257} and {d for *_, d in V.UP} == {1.0, 3.0}
    strides = {s for _, st in V.NOISE for _, s, _ in st}
    assert {6, 15} <= strides and any(len(st) == 3 for _, st in V.NOISE)
    louts = {(s, V.noise_geometry(Lh, s, K)[1]) for Lh, st in V.NOISE for _, s, K in st}
    assert {(6, 1), (15, 1), (15, 2)} <= louts
    assert V.PWG_AUX == (40, 64, 72, 128) and len(V.pwg_cases()) == 8 and V.PWG_REPEAT in V.pwg_cases()
    aux, B, L = V.PWG_SPLITS
    assert V.splits_of(B, V.length(L, S), S) == 12 and aux == 16


# ---- every reference once, on the CPU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', V.dgrad_cases(), ids=V.dgrad_id)
def test_dgrad_references(case):
    tag, C, Cg, K, dil, pad, B, L, form, masked = case
    o = V.dgrad_operands(case)
    d = lambda t: None if t is None else t.double()                             # noqa: E731
    ref = V.dgrad_reference(case, d(o['g']), d(o['w']), d(o['x']), d(o['res']), d(o['sum_in']))
    (dx, bx), (dw, bw), (db, bb) = ref['dx'], ref['dw'], ref['db']
    assert tuple(dx.shape) == tuple(bx.shape) == (B, C, L) and tuple(dw.shape) == tuple(bw.shape) == (Cg, C, K) and tuple(db.shape) == (Cg,)
    assert bool((bx > 0).all()) and bool((bb > 0).all())
    live = V.tap_meets_signal(K, dil, pad, L)
    assert bool(live.any()) and bool((bw[:, :, live] > 0).all()) and float(bw[:, :, ~live].abs().sum()) == 0.0
    if not masked:                               # without the mask the reference is the bare transposed convolution
        want = torch.nn.functional.conv_transpose1d(o['g'].double(), o['w'].double(), padding=pad, dilation=dil)
        assert want.shape == dx.shape and float((want - dx).abs().max()) <= 1e-12


@pytest.mark.parametrize('kind,i', V.wgrad_cases())
def test_wgrad_references(kind, i):
    c = V.wgrad_operands(kind, i, S)
    want, bound = V.wgrad_reference(c, c['g'].double(), c['x'].double())
    assert tuple(want.shape) == ((c['Ci'], c['Co'], c['k']) if kind == 'up' else (c['Co'], c['Ci'], c['k']))
    assert bool((bound > 0).all())
    if kind == 'up':                             # the polyphase view the device writes: rows Co * u, kk columns per input channel
        r, t, kk, ppad = V.taps_of(c['k'], c['u'])
        assert len(r) == len(t) == c['k'] and max(t) < kk and len(set(zip(r, t))) == c['k']


def test_rowsum_up_and_noise_references():
    for B, C, L in V.ROWSUM:
        want, bound = V.rowsum_reference(V.rowsum_operand(B, C, L).double())
        assert tuple(want.shape) == (C,) and bool((bound > 0).all())
    for case in V.UP:
        B, Ci, Co, u, k, L, div = case
        o = V.up_operands(case)
        ref = V.up_reference(case, o['g'].double(), o['x'].double(), o['w'].double())
        assert tuple(ref['dx'][0].shape) == (B, Ci, L) and tuple(ref['dw'][0].shape) == (Ci, Co, k) and tuple(ref['db'][0].shape) == (Co,)
        # tap j of input sample q lands on output q u + j - p: at L = 1 the outer taps of kernel 8 meet no output, and their gradient is exactly 0
        live = torch.tensor([any(0 <= q * u + j - (k - u) // 2 < L * u for q in range(L)) for j in range(k)])
        assert bool((ref['dx'][1] > 0).all()) and bool((ref['db'][1] > 0).all())
        assert bool((ref['dw'][1][:, :, live] > 0).all()) and float(ref['dw'][1][:, :, ~live].abs().sum()) == 0.0
        assert bool(live.all()) == (L > 1)
    for Lh, stages in V.NOISE:
        har, st = V.noise_operands(Lh, stages)
        for s in st:
            assert s['Lo'] >= 1 and tuple(s['g'].shape) == (V.NOISE_B, s['C'], s['Lo'])
            (dw, bw), (db, bb), (dh, bh) = TH.noise_conv_backward(s['g'].double(), har.double(), s['w'].double(), s['s'], s['pad'])
            assert tuple(dw.shape) == (s['C'], s['K']) and tuple(dh.shape) == (V.NOISE_B, Lh) and tuple(db.shape) == (s['C'],)
            # tap j of output n reads har[n s - pad + j]: a weight gradient is live where some output's tap is inside the signal
            live = torch.tensor([any(0 <= n * s['s'] - s['pad'] + j < Lh for n in range(s['Lo'])) for j in range(s['K'])])
            assert bool((bw[:, live] > 0).all()) and float(bw[:, ~live].abs().sum()) == 0.0 and bool((bb > 0).all())


@pytest.mark.parametrize('aux', V.PWG_AUX + (V.PWG_SPLITS[0],))
def test_pwg_references(aux):
    B, L, dil = V.PWG_BLOCK if aux != V.PWG_SPLITS[0] else (V.PWG_SPLITS[1], V.length(V.PWG_SPLITS[2], S), 1)
    o = V.pwg_operands(aux, B, L)
    w = o['w']
    assert float(o['a'].abs().max()) <= V.GATE_RANGE
    d = lambda t: t.double()                                                    # noqa: E731
    a, ab = V.pwg_forward_reference(w, d(o['x']), d(o['c']), dil)
    assert tuple(a.shape) == (B, 128, L) and bool((ab > 0).all())
    da, bda = PH.gate_backward(d(o['dxp']), d(o['dS']), d(o['a']), w['wo'].double(), w['ws'].double())
    assert tuple(da.shape) == (B, 128, L) and bool((bda > 0).all())
    for prev in (None, d(o['dc_prev'])):
        (dx, bx), (dc, bc) = PH.conv_backward(da, d(o['dxp']), w['wc'].double(), w['wa'].double(), dil, prev)
        assert tuple(dx.shape) == (B, 64, L) and tuple(dc.shape) == (B, aux, L) and bool((bx > 0).all()) and bool((bc > 0).all())
    (dw, bw), (db, bb) = PH.wgrad_conv(da, d(o['x']), d(o['c']), dil)
    assert tuple(dw.shape) == (128, 192 + aux) and tuple(db.shape) == (128,) and bool((bw > 0).all()) and bool((bb > 0).all())
    (dw, bw), _ = PH.wgrad_out(d(o['dxp']), d(o['dS']), d(o['a']))
    assert tuple(dw.shape) == (128, 64) and bool((bw > 0).all())
    (dw, bw), _ = PH.wgrad_relu(d(o['g']), d(o['saved']))
    assert tuple(dw.shape) == (64, 64) and bool((bw > 0).all())


def test_restated_bugs_exceed_the_bound():
    """Three bugs these tables are for, restated inside the float64 model on the GPU test's own operands: (a) the channels of the last slab of a
    multi-slab case are dropped from dx; (b) k_split_reduce stops after its unrolled body of 8 splits; (c) k_hgt_rowsum_reduce makes one pass
    over its partials (the first 256).  Each exceeds the bound by at least 100 x wherever it can be seen - except (c) at 257 partials, where the
    lost partial is ONE sample of 262 145: about 4 x - and is the exact result where it cannot (one slab, 8 splits, 256 partials)."""
    seen = {'slab': 0, 'split': 0, 'partial': 0}
    for case in V.dgrad_cases():
        tag, C, Cg, K, dil, pad, B, L, form, masked = case
        slabs = V.dgrad_dispatch(C, Cg, K, dil, pad)['slabs']
        if B != 2 or form != 'first' or not masked or len(slabs) == 1:
            continue
        o = V.dgrad_operands(case)
        g, w, x = o['g'].double(), o['w'].double(), o['x'].double()
        want, bound = V.dgrad_reference(case, g, w, x, None, None)['dx']
        g[:, Cg - slabs[-1]:] = 0
        ratio = E.used(V.dgrad_reference(case, g, w, x, None, None)['dx'][0], want, bound)
        assert ratio >= 100.0, (V.dgrad_id(case), ratio)
        seen['slab'] += 1
    for kind, i in V.wgrad_cases():
        c = V.wgrad_operands(kind, i, S)
        g, x = c['g'].double(), c['x'].double()
        want, bound = V.wgrad_reference(c, g, x)
        nch = (c['L'] + S - 1) // S
        for b in range(c['B']):
            for ch in range(nch):
                if b * nch + ch >= 8:
                    g[b, :, ch * S * c['u']:(ch + 1) * S * c['u']] = 0
        ratio = E.used(V.wgrad_reference(c, g, x)[0], want, bound)
        if V.splits_of(c['B'], c['L'], S) > 8:
            assert ratio >= 100.0, (kind, i, ratio)
            seen['split'] += 1
        else:
            assert ratio == 0.0
    for B, C, L in V.ROWSUM:
        g = V.rowsum_operand(B, C, L).double()
        want, bound = V.rowsum_reference(g)
        nch = (L + V.SUM_CHUNK - 1) // V.SUM_CHUNK
        for b in range(B):
            for ch in range(nch):
                if b * nch + ch >= 256:
                    g[b, :, ch * V.SUM_CHUNK:(ch + 1) * V.SUM_CHUNK] = 0
        ratio = E.used(g.sum((0, 2)), want, bound)
        if V.partials_of(B, L) > 256:
            assert ratio >= (100.0 if V.partials_of(B, L) > 257 else 2.0), ((B, C, L), ratio)
            seen['partial'] += 1
        else:
            assert ratio == 0.0
    print(seen)
    assert seen['slab'] >= 8 and seen['split'] == 2 and seen['partial'] == 2


def test_module_configurations_reach_the_wide_builds():
    h = TH.config(**V.V3)
    convs = V.module_convolutions(h)
    tags = {ch: V.dgrad_dispatch(ch, ch, k, d, p) for ch, k, d, p in convs if (k, d) == (7, 12)}
    assert tags[64]['tag'] == '<2,2>wide' and tags[32]['tag'] == '<4,4>wide' and tags[32]['slabs'] == [24, 8] and tags[16]['tag'] == '<4,4>wide'
    assert TH.hop_of(h) == 256 and set(TH.module_shapes(TH.config(use_pitch_embed=True, **V.V3))) > set(TH.module_shapes(h))
    from tests.test_gpu_voc_edges import ODD
    odd = TH.config(**V.ODD)
    assert all(ODD[k] == odd[k] for k in odd if k != 'use_pitch_embed') and TH.hop_of(odd) == 30
    # the noise strides of the odd configuration are the non-power-of-two strides of TABLE NOISE's first rows
    assert 6 in {s for _, st in V.NOISE for _, s, _ in st}
