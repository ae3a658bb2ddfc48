"""CPU: the yardsticks of tests/test_gpu_voc_edges.py are what they claim to be, and the bound they set catches the bugs it is for.

  * the case tables of tests/voc_edge_helpers.py hold, for every instantiation of k_voc_conv, one length below the reach of the taps, the
    workgroup span and one sample either side of it, and - wherever the channel slab is stated - one Ci that is one 8-group over the slab and
    one that is 4 over (nc8 > nc); the instantiation is derived from the host dispatch's own arithmetic, restated in the helper;
  * the float64 restatements (the tile WALK of conv64 on the case's own geometry, fold64, noise_conv64, pwg_layer64, pwg_upsample64,
    pwg_first64) agree with F.conv1d / F.conv_transpose1d / the oracle in float64 to 1e-12 at every case of the tables - up = 3, 5, 6 through
    `polyphase_weight` at L = 1, 2, 31, 33 included;
  * the float32 CPU evaluation of every case uses at most 0.5 of `bound` (measured: at most 0.40, on the folded form), so the bound is not the loose side;
  * five restated bugs - (a) the left halo of every workgroup span after the first reads zero, (b) the channels of a remainder slab are
    dropped, (c) at up > 1 the phase of the last, partial 32-row block is written one sample late, (d) samples [L, LS) keep their value
    before masking, (e) folded column 256 takes the group of column 255 - exceed the bound by at least 100 x at every case where they can be
    seen at all (no fewer than two each), and are the exact convolution at every other case."""
import pytest
import torch
import torch.nn.functional as F

from diffsinger_amd.vocoder import fold_weight
from oracle import pwg_oracle as PO
from tests import voc_edge_helpers as E
from tests.voc_helpers import HeaderFormulaOps

EMU = HeaderFormulaOps()


def _lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def _torch64(c, kw):
    """the module's own expression in float64: F.conv1d, or F.conv_transpose1d on the ORIGINAL weight, with the fused neighbours"""
    x = _lrelu(c['x'].double(), kw['slope'])
    if c['up'] == 1:
        y = F.conv1d(x, c['w'].double(), c['bias'].double(), padding=c['pad'], dilation=c['dil'])
    else:
        u, k = c['up'], c['wt'].shape[2]
        y = F.conv_transpose1d(x, c['wt'].double(), c['bias'].double(), stride=u, padding=(k - u) // 2)
    if kw['res'] is not None:
        y = y + kw['res'].double()
    if kw['sum_in'] is not None:
        y = kw['sum_in'].double() + y
    y = y / float(torch.tensor(kw['divide'], dtype=torch.float32))
    return E.cm(torch.tanh(y) if kw['act'] else y)


def _cpu32(c, kw):
    Lo = c['L'] * c['up']
    p = lambda t: None if t is None else E.cm(t, Lo)
    return EMU.conv(E.cm(c['x']), c['L'], c['w'], c['bias'], c['rows'], c['x'].shape[1], c['w'].shape[2], c['pad'], c['dil'], up=c['up'],
                    pre_slope=kw['slope'], residual=p(kw['res']), sum_in=p(kw['sum_in']), divide=kw['divide'], act=kw['act'])


def _judge(c, geom, fused=tuple(E.FUSED)):
    """restatement == torch in float64; float32 CPU evaluation within half the bound; returns the largest share"""
    worst = 0.0
    core = {}
    for name in fused:
        kw = E.fused_kw(c, name)
        if kw['slope'] not in core:
            core[kw['slope']] = E.contract64(c['x'], c['w'], c['pad'], c['dil'], c['up'], kw['slope'], geom)
        want, bound = E.conv64(c['x'], c['w'], c['bias'], c['pad'], c['dil'], c['up'], core=core[kw['slope']], **kw)
        ref = _torch64(c, kw)
        assert want.shape == ref.shape
        assert float((want - ref).abs().max()) <= 1e-12, (name, float((want - ref).abs().max()))
        Lo = c['L'] * c['up']
        assert float(want[:, :, Lo:].abs().max() if want.shape[2] > Lo else 0) == 0 and float(bound[:, :, Lo:].abs().max() if want.shape[2] > Lo else 0) == 0
        assert bool((bound[:, :, :Lo] > 0).all())
        share = E.used(_cpu32(c, kw), want, bound)
        assert share <= 0.5, (name, share)
        worst = max(worst, share)
    return worst


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------
def test_geometry_restates_the_kernel_constants():
    for name, (nb, wt, halo) in {'<4,4>': (4, 4, 28), '<2,2>': (2, 2, 28), '<1,1>': (1, 1, 28), '<4,4>wide': (4, 4, 48), '<2,2>wide': (2, 2, 48),
                                 '<1,1>wide': (1, 1, 48), '<4,1>': (4, 1, 28)}.items():
        assert E.slab_of(nb, wt, halo) == E.SLABS[name] and E.span_of(nb, wt) == E.SPANS[name]
    assert E.span_of(2, 4) == E.SPANS['lean<2,4>'] == 256


def test_plain_table_holds_the_edges_of_every_instantiation():
    seen = set()
    for tag, co, k, dil, cis, lengths in E.PLAIN:
        reach = (k - 1) * dil // 2
        for ci in cis:
            for L in lengths:
                assert E.instantiation(2, ci, co, k, reach, dil, L, 1)[0] == tag
        seen.add(tag)
        span, slab = E.SPANS[tag], E.SLABS[tag]
        assert any(L < reach for L in lengths) and 1 in lengths
        assert {span - 1, span, span + 1} <= set(lengths)
        assert slab + 8 in cis and slab + 4 in cis
    assert seen == {'<4,4>', '<2,2>', '<1,1>', '<4,4>wide', '<2,2>wide', '<1,1>wide'}
    for wide in ('<4,4>wide', '<2,2>wide', '<1,1>wide'):                   # each wide build at kernel 7 and at kernel 9, dilation 12
        assert sorted((k - 1) * dil // 2 for tag, _, k, dil, _, _ in E.PLAIN if tag == wide) == [36, 48]
    assert {co for co, *_ in E.SMALL_ROWS} == {1, 5, 20}


def test_transposed_tall_and_lean_tables():
    assert {(u, k) for u, k, _, _ in E.TRANSPOSED} == {(2, 4), (3, 7), (4, 8), (5, 11), (6, 12), (8, 16)}
    assert {E.store_path(u) for u, *_ in E.TRANSPOSED} == {'general', '8-byte', '16-byte'}
    for u in (2, 3, 4, 5, 6, 8):
        rows = sorted(co * uu for uu, _, co, _ in E.TRANSPOSED if uu == u)
        assert len(rows) == 2 and rows[0] < 32 and 33 <= rows[1] <= 64 and rows[1] % 32 != 0
    for u, k, co, ci in E.TRANSPOSED:
        lengths = E.transposed_lengths(u, k, co, ci)
        for L in lengths:
            name, span, _, _ = E.transposed_geometry(u, k, co, ci, L)
            assert name == ('lean<2,4>' if (u == 2 and co * u <= 32) else '<4,4>' if co * u <= 32 else '<2,2>')
            assert {1, 2, 31, 32, 33, span - 1, span, span + 1} == set(lengths)
        assert set(E.ODD_UP_HOST_LENGTHS) <= set(lengths)
    # the tall build: the first call of each pair crosses the 512-workgroup threshold of the dispatch, the B = 2 call does not
    for ci, rows, K, up, B, L in E.TALL:
        assert rows > 64 and E.tall_workgroups(B, rows, L) >= 512 and E.tall_workgroups(2, rows, L) < 512
        assert E.instantiation(B, ci, rows, K, 1, 1, L, up)[0] == '<4,1>' and E.instantiation(2, ci, rows, K, 1, 1, L, up)[0] == '<1,1>'
        assert B % E.TALL_DISTINCT == 0
    assert {ci for ci, *_ in E.TALL} >= {8, E.SLABS['<4,1>'] + 8, E.SLABS['<4,1>'] + 4}
    assert {255, 256, 257, 1, 31, 513} == set(E.LEAN_LENGTHS)
    for ci, co in E.LEAN:
        assert E.transposed_geometry(2, 4, co, ci, 256)[0] == 'lean<2,4>' and E.transposed_geometry(2, 4, co, ci, 256, lean=False)[0] == '<4,4>'


def test_fold_table():
    assert [E.fold_factor_model(co, ci, 3, 1) for co, ci in E.FOLD_SHAPES] == [4, 4, 4, 2, 2]
    assert {(F_, k): E.fold_max_dilation(co, ci, k) for (co, ci), F_ in (((8, 8), 4), ((16, 16), 2)) for k in E.FOLD_KERNELS} == \
        {(4, 3): 8, (4, 7): 6, (4, 11): 5, (2, 3): 12, (2, 7): 8, (2, 11): 5}
    for F_, dil in ((4, 1), (4, 8), (2, 12), (2, 5)):
        ls, p = E.fold_lengths(F_, dil), E.fold_pos(256, F_, dil)
        assert {1, 2, 3, 5, 31, 32, 33, F_ * dil, p - 1, p, p + 1} <= set(ls) and (F_ * dil == 1 or F_ * dil - 1 in ls)
        assert any(L < F_ for L in ls) and any(L < F_ * dil for L in ls)


# ---- restatement == torch, float32 CPU evaluation inside half the bound -----------------------------------------------------------------------
@pytest.mark.parametrize('row', range(len(E.PLAIN)), ids=lambda i: f'{E.PLAIN[i][0]}k{E.PLAIN[i][2]}')
def test_plain_convolutions(row):
    tag, co, k, dil, cis, lengths = E.PLAIN[row]
    worst = 0.0
    for ci in cis:
        for L in lengths:
            c = E.plain_case(co, ci, k, dil, L)
            worst = max(worst, _judge(c, E.instantiation(2, ci, co, k, c['pad'], dil, L, 1)))
    print(f'{tag} k{k} d{dil}: float32 CPU uses at most {worst:.3f} of the bound')


def test_rows_that_fill_no_block():
    for co, ci, k, dil, L in E.SMALL_ROWS:
        c = E.plain_case(co, ci, k, dil, L)
        _judge(c, E.instantiation(2, ci, co, k, c['pad'], dil, L, 1))


@pytest.mark.parametrize('u,k,co,ci', E.TRANSPOSED)
def test_transposed_convolutions_through_the_polyphase_weight(u, k, co, ci):
    worst = 0.0
    for L in E.transposed_lengths(u, k, co, ci):
        c = E.transposed_case(u, k, co, ci, L)
        worst = max(worst, _judge(c, E.transposed_geometry(u, k, co, ci, L), fused=('bare', 'res', 'all')))
    print(f'u{u} k{k} rows {co * u}: float32 CPU uses at most {worst:.3f} of the bound')


@pytest.mark.parametrize('ci,co', E.LEAN)
def test_lean_build_cases(ci, co):
    """the operands of the GPU test's lean cases (B = 3) on the lean build's own walk: span 256, a 4-sample halo"""
    for L in E.LEAN_LENGTHS:
        c = E.transposed_case(2, 4, co, ci, L, B=3)
        geom = E.transposed_geometry(2, 4, co, ci, L)
        assert geom[0] == 'lean<2,4>' and geom[1] == 256 and geom[3] == E.HALO_LEAN
        _judge(c, geom, fused=('res',))


@pytest.mark.parametrize('ci,rows,K,up,B,L', E.TALL)
def test_tall_build_cases(ci, rows, K, up, B, L):
    c = E.transposed_case(up, 16, rows // up, ci, L, B=E.TALL_DISTINCT)
    assert c['w'].shape == (rows, ci, K) and c['pad'] == 1
    _judge(c, E.instantiation(B, ci, rows, K, 1, 1, L, up), fused=('res',))
    big = E.transposed_case(up, 16, rows // up, ci, L, B=B, distinct=E.TALL_DISTINCT)
    assert big['x'].shape[0] == B and torch.equal(big['x'][:E.TALL_DISTINCT], c['x']) and torch.equal(big['x'][E.TALL_DISTINCT:2 * E.TALL_DISTINCT], c['x'])


@pytest.mark.parametrize('co,ci', E.FOLD_SHAPES)
@pytest.mark.parametrize('k', E.FOLD_KERNELS)
def test_folded_convolutions(co, ci, k):
    """fold64 is F.conv1d; the float32 evaluation is the FOLDED formula of the header (tests/voc_helpers.py) on `fold_weight`'s rows"""
    F_ = E.fold_factor_model(co, ci, k, 1)
    worst = 0.0
    for dil in (1, E.fold_max_dilation(co, ci, k)):
        assert E.fold_factor_model(co, ci, k, dil) == F_ and E.fold_factor_model(co, ci, k, E.fold_max_dilation(co, ci, k) + 1) == 1
        for L in E.fold_lengths(F_, dil):
            c = E.plain_case(co, ci, k, dil, L)
            for name in E.FUSED:
                kw = E.fused_kw(c, name)
                want, bound = E.fold64(c['x'], c['w'], c['bias'], F_, dil, **kw)
                assert float((want - _torch64(c, kw)).abs().max()) <= 1e-12
                p = lambda t: None if t is None else E.cm(t, L)
                got = EMU.conv_folded(E.cm(c['x']), L, fold_weight(c['w'], F_), c['bias'], co, ci, k, F_, dil, pre_slope=kw['slope'], residual=p(kw['res']),
                                      sum_in=p(kw['sum_in']), divide=kw['divide'], act=kw['act'])
                share = E.used(got, want, bound)
                assert share <= 0.5, (dil, L, name, share)
                worst = max(worst, share)
    print(f'folded co{co} k{k}: float32 CPU uses at most {worst:.3f} of the bound')


@pytest.mark.parametrize('C,s,K', E.NOISE)
def test_noise_convolution(C, s, K):
    for Lh in E.noise_lengths(s):
        c = E.noise_case(C, s, K, Lh)
        want, bound = E.noise_conv64(c['har'], c['w'], c['bias'], s, c['pad'], c['L_out'])
        ref = F.conv1d(c['har'].double()[:, None], c['w'].double()[:, None], c['bias'].double(), stride=s, padding=c['pad'])
        assert ref.shape[2] == c['L_out'] == {s: 1, 2 * s: 2, 33 * s: 33}.get(Lh, 8192 // s + 1)
        assert float((want[:, :, :c['L_out']] - ref).abs().max()) <= 1e-12
        har = torch.zeros(c['har'].shape[0], E.padded(Lh))
        har[:, :Lh] = c['har']
        assert E.used(EMU.noise_conv(har, Lh, c['w'], c['bias'], s, c['pad'], c['L_out']), want, bound) <= 0.5


def _pwg_params(c, aux):
    p = {'conv.weight': c['w1'][:, :192].reshape(128, 3, 64).permute(0, 2, 1).contiguous(), 'conv.bias': c['b1'],
         'conv1x1_out.weight': c['w2'][:64, :, None], 'conv1x1_out.bias': c['b2'][:64],
         'conv1x1_skip.weight': c['w2'][64:, :, None], 'conv1x1_skip.bias': c['b2'][64:]}
    if aux:
        p['conv1x1_aux.weight'] = c['w1'][:, 192:, None]
    return p


@pytest.mark.parametrize('aux', E.PWG_AUX)
def test_pwg_layer_restatement(aux):
    worst = 0.0
    for L in E.PWG_LENGTHS:
        for dil in E.PWG_DILATIONS:
            for scale in (1.0, 25.0):
                c = E.pwg_case(2, L, aux, scale=scale, observe_gate=scale > 1)
                xo, bx, sk, bs, z = E.pwg_layer64(c['x'], c['c'], c['w1'], c['b1'], c['w2'], c['b2'], dil, prev=c['prev'])
                p = _pwg_params(c, aux)
                xr, sr = PO.residual_block({k: v.double() for k, v in p.items()}, '', c['x'].double(), None if c['c'] is None else c['c'].double(), dil)
                assert float((xo[:, :, :L] - xr).abs().max()) <= 1e-12 and float((sk[:, :, :L] - (c['prev'].double() + sr)).abs().max()) <= 1e-12
                x32, s32 = PO.residual_block(p, '', c['x'], c['c'], dil)
                share = max(E.used(E.cm(x32), xo, bx), E.used(E.cm(c['prev'] + s32), sk, bs))
                assert share <= 0.5, (L, dil, scale, share)
                worst = max(worst, share)
                if scale > 1:
                    at, ag, _, _ = E.pwg_gate64(c['x'], c['c'], c['w1'], c['b1'], dil)
                    assert float(at.abs().max()) >= 100 and float(ag.abs().max()) >= 100
    print(f'pwg layer aux {aux}: float32 CPU uses at most {worst:.3f} of the bound')
    assert any(d >= L for d in E.PWG_DILATIONS for L in E.PWG_LENGTHS) and any(d == L - 1 for d in E.PWG_DILATIONS for L in E.PWG_LENGTHS)


@pytest.mark.parametrize('L,scale', [(1, 4), (33, 2), (33, 8), (70, 4)])
def test_pwg_upsample_and_first(L, scale):
    g = torch.Generator().manual_seed(L * 10 + scale)
    x = torch.randn(2, 5, L, generator=g)
    w = torch.randn(2 * scale + 1, generator=g)
    want, bound = E.pwg_upsample64(x, w, scale)
    up = lambda t: F.conv2d(F.interpolate(t.unsqueeze(1), scale_factor=(1, scale), mode='nearest'), w.to(t.dtype).reshape(1, 1, 1, -1), padding=(0, scale)).squeeze(1)
    assert float((want[:, :, :L * scale] - up(x.double())).abs().max()) <= 1e-12
    assert E.used(E.cm(up(x)), want, bound) <= 0.5
    z, wf, bf = torch.randn(2, L, generator=g), torch.randn(7, generator=g), torch.randn(7, generator=g)
    want, bound = E.pwg_first64(z, wf, bf)
    assert float((want[:, :, :L] - F.conv1d(z.double()[:, None], wf.double()[:, None, None], bf.double())).abs().max()) <= 1e-12
    assert E.used(E.cm(F.conv1d(z[:, None], wf[:, None, None], bf)), want, bound) <= 0.5


# ---- the restated bugs --------------------------------------------------------------------------------------------------------------------------
def _mutant_cases():
    """(case, geometry, fused) over the plain, small-row, transposed and tall tables: the ends and the seams of every row"""
    for tag, co, k, dil, cis, lengths in E.PLAIN:
        span = E.SPANS[tag]
        for ci in cis:
            for L in sorted({lengths[0], span - 1, span, span + 1, max(lengths)} & set(lengths)):
                c = E.plain_case(co, ci, k, dil, L)
                yield c, E.instantiation(2, ci, co, k, c['pad'], dil, L, 1), 'res+sum/3'
    for co, ci, k, dil, L in E.SMALL_ROWS:
        c = E.plain_case(co, ci, k, dil, L)
        yield c, E.instantiation(2, ci, co, k, c['pad'], dil, L, 1), 'tanh'
    for u, k, co, ci in E.TRANSPOSED:
        for L in E.transposed_lengths(u, k, co, ci):
            yield E.transposed_case(u, k, co, ci, L), E.transposed_geometry(u, k, co, ci, L), 'res'
    for ci, rows, K, up, B, L in E.TALL:
        yield E.transposed_case(up, 16, rows // up, ci, L, B=E.TALL_DISTINCT), E.instantiation(B, ci, rows, K, 1, 1, L, up), 'res'


def test_mutants_exceed_the_bound_where_they_are_observable():
    seen = {m: [] for m in E.MUTANTS}
    for c, geom, fused in _mutant_cases():
        kw = E.fused_kw(c, fused)
        ci = c['x'].shape[1]
        want, bound = E.conv64(c['x'], c['w'], c['bias'], c['pad'], c['dil'], c['up'], geom=geom, **kw)
        for m in E.MUTANTS:
            core = E.contract64(c['x'], c['w'], c['pad'], c['dil'], c['up'], kw['slope'], geom, mutant=m, magnitudes=False)
            got, _ = E.conv64(c['x'], c['w'], c['bias'], c['pad'], c['dil'], c['up'], mutant=m, core=core, **kw)
            if E.mutant_seen(m, geom, ci, c['rows'], c['L'], c['up']):
                ratio = E.used(got, want, bound)
                assert ratio >= 100.0, (m, geom[0], ci, c['rows'], c['L'], c['up'], ratio)
                seen[m].append(ratio)
            else:
                assert float((got - want).abs().max()) <= 1e-12, (m, geom[0], ci, c['rows'], c['L'], c['up'])
    for m, r in seen.items():
        print(f'mutant ({m}): seen at {len(r)} cases, at least {min(r):.0f} x the bound')
        assert len(r) >= 2, m


def test_fold_column_mutant():
    ratios = []
    for (co, ci), k in (((8, 8), 3), ((16, 16), 7), ((5, 12), 11)):
        F_ = E.fold_factor_model(co, ci, k, 1)
        for dil in (1, E.fold_max_dilation(co, ci, k)):
            for L in E.fold_lengths(F_, dil):
                c = E.plain_case(co, ci, k, dil, L)
                kw = E.fused_kw(c, 'res')
                want, bound = E.fold64(c['x'], c['w'], c['bias'], F_, dil, **kw)
                got, _ = E.fold64(c['x'], c['w'], c['bias'], F_, dil, mutant='column', **kw)
                if E.fold_mutant_seen(F_, dil, L):
                    ratios.append(E.used(got, want, bound))
                    assert ratios[-1] >= 100.0, (co, k, dil, L, ratios[-1])
                else:
                    assert float((got - want).abs().max()) == 0.0, (co, k, dil, L)
    print(f'mutant (column): seen at {len(ratios)} cases, at least {min(ratios):.0f} x the bound')
    assert len(ratios) >= 2
