"""The vocoder's inference kernels (bench row f2: csrc/voc_kernels.hpp, voc_chain.hpp, pwg_kernels.hpp behind the host dispatch of voc_abi.hpp) on the
MI355X at short lengths, workgroup and channel-slab seams and odd phase counts, through the C ABI of include/dsv.h, against the float64
restatements of tests/voc_edge_helpers.py with element-wise bounds (the bounds themselves are judged on the CPU by tests/test_voc_edges_host.py).

Every output buffer the test hands to the library is pre-filled with NaN; every written tensor must be finite, exactly zero on [L, LS) and within
`bound` element-wise (the bound is 0 on the tail).  Each test prints its largest err / bound ("share").

dsv_conv1d, plain: every instantiation (<4,4>, <2,2>, <1,1> and their wide builds) at lengths below the reach of the taps, at the workgroup span
and one sample either side of it, with a Ci one 8-group and one half group over the channel slab, rows that fill no block, and every fused
neighbour at every length.  Transposed: up = 2, 3, 4, 5, 6, 8 (the general, 8-byte and 16-byte store paths), rows below 32 and 33..64 with a
partial last block, residual and residual + sum_in + divide + tanh at every length, against float64 conv_transpose1d.  The tall build <4,1> at
the dispatch threshold (asserted from the rule's own arithmetic), against conv64 and bit for bit against the <1,1> build of a B = 2 call.  The
lean build against dsv_set_lean(0) bit for bit.  dsv_conv1d_folded against the PLAIN convolution at dilation 1 and the largest dilation the
library folds, lengths below F and F dil and around the 256-column seam.  Chains and dsv_conv1d_multi bit for bit against single launches at
L = 1 .. 33, a wide-reach group among narrow ones included.  dsv_noise_conv at one and two outputs and across a 256-thread block.  One whole
generator with phase counts 5, 3, 2.  dsv_pwg_layer at L <= 97 with dil >= L, n_aux up to 128 and saturated gates; dsv_pwg_upsample, dsv_pwg_first.

LEFT OUT, with the reason: the whole generator at upsample_rates [5, 3, 2] WITH the NSF source.  HifiGanGenerator.forward refuses a hop that is
not a power of two when f0 is given (k_voc_sine reads frame index // hop; torch's nearest upsampling is exact against that for powers of two
only) - a deliberate refusal of the module, pinned here as such (test_odd_phase_generator_refuses_the_source_at_hop_30); k_voc_sine and
k_voc_source have their own model (tests/voc_helpers.chunked_sine).  The table conditions of the host test do not involve this case.

MEASURED on the MI355X, 2026-10-20 (every case passes; no kernel was changed).  "share" = largest |device - float64| / bound over the elements of
every case of the line; per fused neighbour as bare / res / res+sum/3 / tanh / all (transposed: res / all).
  dsv_conv1d, plain (each wide build at kernel 7 and at kernel 9, dilation 12, with the full Ci and L sets):
      <4,4> k11 d5      0.431 / 0.421 / 0.419 / 0.240 / 0.274        <4,4>wide k7 d12  0.318 / 0.317 / 0.328 / 0.222 / 0.230
      <2,2> k7 d5       0.375 / 0.354 / 0.340 / 0.325 / 0.290        <4,4>wide k9 d12  0.443 / 0.379 / 0.360 / 0.218 / 0.265
      <1,1> k7 d1       0.363 / 0.354 / 0.335 / 0.309 / 0.323        <2,2>wide k7 d12  0.341 / 0.343 / 0.325 / 0.229 / 0.238
      rows 1, 5, 20     0.269 / 0.218 / 0.236 / 0.152 / 0.184        <2,2>wide k9 d12  0.345 / 0.338 / 0.325 / 0.291 / 0.240
                                                                     <1,1>wide k7 d12  0.323 / 0.280 / 0.261 / 0.262 / 0.263
                                                                     <1,1>wide k9 d12  0.378 / 0.317 / 0.309 / 0.272 / 0.291
  dsv_conv1d, transposed (u, k: rows below 32 | rows 33..64):
      2, 4 (8-byte, lean<2,4> | <2,2>)   0.209 / 0.112 | 0.262 / 0.140      3, 7 (general)    0.230 / 0.157 | 0.255 / 0.180
      4, 8 (16-byte)                     0.237 / 0.131 | 0.228 / 0.158      5, 11 (general)   0.364 / 0.163 | 0.257 / 0.128
      8, 16 (16-byte)                    0.252 / 0.145 | 0.246 / 0.159      6, 12 (general)   0.209 / 0.165 | 0.194 / 0.143
  the tall build <4,1>, B 128: Ci 8 0.208, Ci 104 0.394, Ci 100 0.286; the bits of <1,1> at B 2 in every case
  the lean build lean<2,4>: Ci 16 0.209, Ci 32 0.253, Ci 8 0.178; the bits of the standard build at every length
  dsv_conv1d_folded, largest over Co and both dilations, per kernel size:
      k3 0.326 / 0.281 / 0.287 / 0.194 / 0.183     k7 0.359 / 0.366 / 0.288 / 0.218 / 0.195     k11 0.348 / 0.331 / 0.274 / 0.256 / 0.230
  chains (stages 1 - 3, six modes, L = 1, 5, 31, 32) and dsv_conv1d_multi (three tilings, L = 1, 31, 33, wide among narrow): the same bits
  dsv_noise_conv: (64, 32, 64) 0.239, (16, 2, 4) 0.134, (8, 1, 1) 0.078, (32, 6, 12) 0.172
  whole generator [5, 3, 2] without the source, B 2, T 7: max err 5.1e-7; allowed 1.7e-6 = 4 x the float32 oracle's 4.3e-7 (RULE max|y| = 6.9e-7)
  dsv_pwg_layer: n_aux 0 / 8 / 80 / 128: 0.010 / 0.010 / 0.007 / 0.007; gates beyond +-250: 0.059 and 0.036, saturation exact
  the PWG gate allowance (16 U), on exact pre-activations over +-16: |z - z64| = 2.4e-7 = 3.97 U = 0.248 of the allowance
  dsv_pwg_upsample <= 0.165, dsv_pwg_first <= 0.062
"""
import os

import pytest
import torch
import torch.nn.functional as F

from diffsinger_amd import _lib
from diffsinger_amd.vocoder import DsvConvDesc, HifiGanGenerator, _HipOps, fold_weight, padded_samples
from oracle import hifigan_oracle as HO
from oracle.make_golden_hifigan import CONFIG
from tests import voc_edge_helpers as E
from tests.test_gpu_vocoder import _cm, _generator, chain_default  # noqa: F401  (chain_default is a fixture)
from tests.voc_helpers import draws_like_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def _conv1d(ops, x, L, wp, bias, rows, ci, k, pad, dil, up=1, slope=1.0, res=None, sum_in=None, divide=1.0, act=0):
    """dsv_conv1d into a NaN-filled buffer; x, res, sum_in: device tensors in the padded layout"""
    B = x.shape[0]
    assert x.shape == (B, ci, padded_samples(L)) and x.is_contiguous()
    out = _nan(B, rows // up, padded_samples(L * up))
    _lib.check(ops.lib.dsv_conv1d(x.data_ptr(), wp.data_ptr(), _p(bias), out.data_ptr(), B, ci, rows, k, pad, dil, L, up, float(slope), _p(res), _p(sum_in),
                                  float(divide), int(act), _stream()), 'dsv_conv1d')
    return out


def _folded(ops, x, L, wp, bias, co, ci, k, F_, dil, slope=1.0, res=None, sum_in=None, divide=1.0, act=0):
    B = x.shape[0]
    out = _nan(B, co, padded_samples(L))
    _lib.check(ops.lib.dsv_conv1d_folded(x.data_ptr(), wp.data_ptr(), _p(bias), out.data_ptr(), B, ci, co, k, F_, dil, L, float(slope), _p(res), _p(sum_in),
                                         float(divide), int(act), _stream()), 'dsv_conv1d_folded')
    return out


def _share(got, want, bound, Lo):
    """finite, zero tail, element-wise bound -> err / bound"""
    got = got.cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), 'an element was not written (NaN pre-fill) or is not finite'
    if got.shape[-1] > Lo:
        assert float(got[..., Lo:].abs().max()) == 0.0
    return E.used(got, want, bound)


def _run_case(ops, c, fused_names):
    """one shape through every fused neighbour of `fused_names` -> {name: share}"""
    L, up, Lo = c['L'], c['up'], c['L'] * c['up']
    x = _d(E.cm(c['x']))
    wp = ops.pack(_d(c['w']))
    bias = _d(c['bias'])
    res, acc = _d(E.cm(c['res'], Lo)), _d(E.cm(c['acc'], Lo))
    core, out = {}, {}
    for name in fused_names:
        kw = E.fused_kw(c, name)
        if kw['slope'] not in core:
            core[kw['slope']] = E.contract64(c['x'], c['w'], c['pad'], c['dil'], up, kw['slope'])
        want, bound = E.conv64(c['x'], c['w'], c['bias'], c['pad'], c['dil'], up, core=core[kw['slope']], **kw)
        got = _conv1d(ops, x, L, wp, bias, c['rows'], c['x'].shape[1], c['w'].shape[2], c['pad'], c['dil'], up, kw['slope'],
                      res if kw['res'] is not None else None, acc if kw['sum_in'] is not None else None, kw['divide'], kw['act'])
        out[name] = _share(got, want, bound, Lo)
    return out


def _report(tag, shares):
    """shares: {fused name: [share, ...]}"""
    txt = '   '.join(f'{n} {max(v):.3f}' for n, v in shares.items())
    print(f'EDGE {tag}: share of the bound per fused neighbour: {txt}')
    for n, v in shares.items():
        assert max(v) <= 1.0, (tag, n, max(v))


# ---- dsv_conv1d, plain --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', range(len(E.PLAIN)), ids=lambda i: f'{E.PLAIN[i][0]}k{E.PLAIN[i][2]}')
def test_plain_convolution(row):
    tag, co, k, dil, cis, lengths = E.PLAIN[row]
    ops = _HipOps()
    shares = {n: [] for n in E.FUSED}
    for ci in cis:
        for L in lengths:
            for n, s in _run_case(ops, E.plain_case(co, ci, k, dil, L), E.FUSED).items():
                assert s <= 1.0, (tag, ci, L, n, s)
                shares[n].append(s)
    _report(f'conv1d {tag} k{k} d{dil} Ci {cis} L {lengths}', shares)


def test_rows_that_fill_no_block():
    ops = _HipOps()
    shares = {n: [] for n in E.FUSED}
    for co, ci, k, dil, L in E.SMALL_ROWS:
        for n, s in _run_case(ops, E.plain_case(co, ci, k, dil, L), E.FUSED).items():
            assert s <= 1.0, (co, L, n, s)
            shares[n].append(s)
    _report('conv1d rows 1, 5, 20 at Ci 12', shares)


# ---- dsv_conv1d, transposed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('u,k,co,ci', E.TRANSPOSED)
def test_transposed_convolution(u, k, co, ci):
    ops = _HipOps()
    shares = {'res': [], 'all': []}
    lengths = E.transposed_lengths(u, k, co, ci)
    for L in lengths:
        c = E.transposed_case(u, k, co, ci, L)
        # float64 conv_transpose1d on the module's weight is what conv64 restates (to 1e-12 on the CPU; once more here at the first length)
        if L == lengths[0]:
            x = E.lrelu64(c['x'], 0.1)
            ref = F.conv_transpose1d(x, c['wt'].double(), c['bias'].double(), stride=u, padding=(k - u) // 2)
            want, _ = E.conv64(c['x'], c['w'], c['bias'], c['pad'], 1, u, slope=0.1)
            assert float((want[:, :, :L * u] - ref).abs().max()) <= 1e-12
        for n, s in _run_case(ops, c, ('res', 'all')).items():
            assert s <= 1.0, (u, k, co, L, n, s)
            shares[n].append(s)
    _report(f'transposed u{u} k{k} rows {co * u} ({E.store_path(u)} stores, {E.transposed_geometry(u, k, co, ci, lengths[-1])[0]}) L {lengths}', shares)


# ---- the tall build ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci,rows,K,up,B,L', E.TALL)
def test_tall_build(ci, rows, K, up, B, L):
    """<4,1> is chosen when rows > 64 and ceil(LSi / 128) * B * ceil(rows / 128) >= 512 (csrc/voc_abi.hpp): the B = 128 call crosses that, the B = 2
    call of the same utterances does not and runs <1,1>.  Same chunk order, same bits - and both within the bound of conv64."""
    LS = padded_samples(L)
    wgs = lambda b: ((LS + 127) // 128) * b * ((rows + 127) // 128)
    assert rows > 64 and wgs(B) >= 512 and wgs(2) < 512
    ops = _HipOps()
    nd = E.TALL_DISTINCT
    c = E.transposed_case(up, 16, rows // up, ci, L, B=B, distinct=nd)
    assert c['w'].shape == (rows, ci, K) and c['x'].shape[0] == B
    Lo = L * up
    x, res = _d(E.cm(c['x'])), _d(E.cm(c['res'], Lo))
    wp, bias = ops.pack(_d(c['w'])), _d(c['bias'])
    got = _conv1d(ops, x, L, wp, bias, rows, ci, K, c['pad'], 1, up, 0.1, res)
    want, bound = E.conv64(c['x'][:nd], c['w'], c['bias'], c['pad'], 1, up, slope=0.1, res=c['res'][:nd])
    share = _share(got[:nd], want, bound, Lo)
    assert torch.equal(got, got[:nd].repeat(B // nd, 1, 1)), 'a repeated utterance does not carry the bits of its first copy'
    assert bool(torch.isfinite(got).all()) and (got.shape[2] == Lo or float(got[:, :, Lo:].abs().max()) == 0.0)
    for b0 in range(0, nd, 2):
        two = _conv1d(ops, x[b0:b0 + 2].contiguous(), L, wp, bias, rows, ci, K, c['pad'], 1, up, 0.1, res[b0:b0 + 2].contiguous())
        assert torch.equal(two, got[b0:b0 + 2]), float((two - got[b0:b0 + 2]).abs().max())
    print(f'EDGE conv1d <4,1> Ci {ci} rows {rows} B {B} L {L}: uses {share:.3f} of the bound; the bits of <1,1> at B = 2')
    assert share <= 1.0


# ---- the lean build ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci,co', E.LEAN)
def test_lean_build(ci, co):
    # voc_lean_try (csrc/voc_abi.hpp) also reads the environment once: with DSV_LEAN=0 both launches below would run the standard build and the
    # comparison would compare it with itself
    assert int(os.environ.get('DSV_LEAN', '1')) != 0, 'DSV_LEAN disables the lean build: this test would not run it'
    lib = _lib.load()
    ops = _HipOps()
    shares = []
    for L in E.LEAN_LENGTHS:
        c = E.transposed_case(2, 4, co, ci, L, B=3)
        assert E.transposed_geometry(2, 4, co, ci, L)[0] == 'lean<2,4>'
        x, wp, bias, res = _d(E.cm(c['x'])), ops.pack(_d(c['w'])), _d(c['bias']), _d(E.cm(c['res'], 2 * L))
        args = (x, L, wp, bias, c['rows'], ci, c['w'].shape[2], c['pad'], 1, 2, 0.1, res)
        try:
            assert lib.dsv_set_lean(0) == 0
            std = _conv1d(ops, *args)
            assert lib.dsv_set_lean(1) == 0
            lean = _conv1d(ops, *args)
            torch.cuda.synchronize()
        finally:
            lib.dsv_set_lean(1)
        want, bound = E.conv64(c['x'], c['w'], c['bias'], c['pad'], 1, 2, slope=0.1, res=c['res'])
        shares.append(_share(lean, want, bound, 2 * L))
        assert torch.equal(lean, std), (L, float((lean - std).abs().max()))
    print(f'EDGE conv1d lean<2,4> Ci {ci} rows {2 * co} L {E.LEAN_LENGTHS}: uses {max(shares):.3f} of the bound; the bits of the standard build')
    assert max(shares) <= 1.0


# ---- dsv_conv1d_folded ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fold_on():
    lib = _lib.load()
    lib.dsv_set_fold(1)
    yield lib
    lib.dsv_set_fold(1)


@pytest.mark.parametrize('co,ci', E.FOLD_SHAPES)
@pytest.mark.parametrize('k', E.FOLD_KERNELS)
def test_folded_convolution(co, ci, k, fold_on):
    ops = _HipOps()
    F_ = 4 if co <= 8 else 2
    dmax = 1
    while ops.fold_factor(co, ci, k, dmax + 1) == F_:                  # the largest dilation the LIBRARY still folds
        dmax += 1
    assert ops.fold_factor(co, ci, k, 1) == F_ and dmax == E.fold_max_dilation(co, ci, k) and dmax > 1
    shares = {n: [] for n in E.FUSED}
    for dil in (1, dmax):
        for L in E.fold_lengths(F_, dil):
            c = E.plain_case(co, ci, k, dil, L)
            x, wp, bias = _d(E.cm(c['x'])), ops.pack(_d(fold_weight(c['w'], F_))), _d(c['bias'])
            res, acc = _d(E.cm(c['res'])), _d(E.cm(c['acc']))
            core = {}
            for n in E.FUSED:
                kw = E.fused_kw(c, n)
                if kw['slope'] not in core:
                    core[kw['slope']] = E.contract64(c['x'], c['w'], c['pad'], dil, 1, kw['slope'])
                want, bound = E.fold64(c['x'], c['w'], c['bias'], F_, dil, core=core[kw['slope']], **kw)
                got = _folded(ops, x, L, wp, bias, co, ci, k, F_, dil, kw['slope'], res if kw['res'] is not None else None,
                              acc if kw['sum_in'] is not None else None, kw['divide'], kw['act'])
                s = _share(got, want, bound, L)
                assert s <= 1.0, (co, k, dil, L, n, s)
                shares[n].append(s)
    _report(f'folded F{F_} Co {co} k{k} d 1 / {dmax}', shares)


# ---- chains and dsv_conv1d_multi: bit for bit against single launches -----------------------------------------------------------------------------
@pytest.mark.parametrize('stage', [1, 2, 3])
@pytest.mark.parametrize('mode', ['stage', 'resblock', 'pair', 'merged0', 'merged1', 'merged2'])
def test_resblock_chains_at_short_lengths(stage, mode, chain_default):
    """the comparison of test_gpu_vocoder.test_resblock_chain_is_bit_identical_to_the_single_convolutions at lengths inside one 32-sample block"""
    h, p, m = _generator(dict(nsf=False, B=2, T=8, seed=41 + stage))
    m(torch.zeros(1, 80, 4, device=DEV))
    C = 128 >> (stage + 1)
    for L in (1, 5, 31, 32):
        g = torch.Generator().manual_seed(100 * stage + L)
        x = _cm(torch.randn(3, C, L, generator=g), L).to(DEV)
        chain_default.set_chain_mode('off')
        want = m._stage_resblocks(stage, x, L)
        chain_default.set_chain_mode(mode)
        got = m._stage_resblocks(stage, x, L)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()) and float(got[:, :, L:].abs().max() if got.shape[2] > L else 0) == 0
        assert float(want.abs().max()) > 0
        assert torch.equal(got, want), (L, float((got - want).abs().max()))


def _multi(ops, xs, L, items, slope):
    """dsv_conv1d_multi into NaN-filled buffers"""
    B, rows, ci = xs[0].shape[0], items[0]['rows'], items[0]['ci']
    outs, descs = [], (DsvConvDesc * len(xs))()
    for g, (x, it) in enumerate(zip(xs, items)):
        outs.append(_nan(B, rows, padded_samples(L)))
        descs[g] = DsvConvDesc(x.data_ptr(), it['wp'].data_ptr(), _p(it.get('bias')), outs[g].data_ptr(), _p(it.get('residual')), _p(it.get('sum_in')),
                               it['k'], it['pad'], it['dil'], 0, float(it.get('divide', 1.0)), 0)
    _lib.check(ops.lib.dsv_conv1d_multi(len(xs), descs, B, ci, rows, L, 1, float(slope), _stream()), 'dsv_conv1d_multi')
    return outs


@pytest.mark.parametrize('C', [32, 64, 128])
@pytest.mark.parametrize('kinds', [((11, 5), (7, 3), (3, 1)), ((7, 12), (3, 1), (11, 1))], ids=['narrow', 'wide-among-narrow'])
def test_conv1d_multi_at_short_lengths(C, kinds):
    """three groups in one launch against three dsv_conv1d launches; 'wide-among-narrow': kernel 7 at dilation 12 (reach 36) forces EVERY group
    onto the +-48-sample instantiation while its own single launch of a narrow group runs the +-28 one - the same bits are claimed for that"""
    ops = _HipOps()
    for L in (1, 31, 33):
        g = torch.Generator().manual_seed(C + L)
        B = 2
        xs, items, raw = [], [], []
        for k, dil in kinds:
            w = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
            x = torch.randn(B, C, L, generator=g)
            b = torch.randn(C, generator=g)
            raw.append((x, w, b, k, dil))
            xs.append(_d(E.cm(x)))
            items.append(dict(wp=ops.pack(_d(w)), bias=_d(b), rows=C, ci=C, k=k, pad=(k - 1) * dil // 2, dil=dil))
        r1, r2, s2 = (torch.randn(B, C, L, generator=g) for _ in range(3))
        items[1]['residual'] = _d(E.cm(r1))
        items[2]['residual'], items[2]['sum_in'], items[2]['divide'] = _d(E.cm(r2)), _d(E.cm(s2)), 3.0
        single = [_conv1d(ops, x, L, it['wp'], it['bias'], C, C, it['k'], it['pad'], it['dil'], 1, 0.1, it.get('residual'), it.get('sum_in'), it.get('divide', 1.0))
                  for x, it in zip(xs, items)]
        got = _multi(ops, xs, L, items, 0.1)
        torch.cuda.synchronize()
        extras = [dict(), dict(res=r1), dict(res=r2, sum_in=s2, divide=3.0)]
        for i, (a, b) in enumerate(zip(got, single)):
            x, w, bb, k, dil = raw[i]
            want, bound = E.conv64(x, w, bb, (k - 1) * dil // 2, dil, 1, slope=0.1, **extras[i])
            assert _share(a, want, bound, L) <= 1.0
            assert torch.equal(a, b), (C, L, i, float((a - b).abs().max()))


# ---- dsv_noise_conv ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,s,K', E.NOISE)
def test_noise_convolution(C, s, K):
    ops = _HipOps()
    shares = []
    for Lh in E.noise_lengths(s):
        c = E.noise_case(C, s, K, Lh)
        B = c['har'].shape[0]
        har = torch.zeros(B, padded_samples(Lh))
        har[:, :Lh] = c['har']
        out = _nan(B, C, padded_samples(c['L_out']))
        hd, wd, bd = _d(har), _d(c['w']), _d(c['bias'])
        _lib.check(ops.lib.dsv_noise_conv(hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, C, K, s, c['pad'], Lh, c['L_out'], _stream()), 'dsv_noise_conv')
        want, bound = E.noise_conv64(c['har'], c['w'], c['bias'], s, c['pad'], c['L_out'])
        shares.append(_share(out, want, bound, c['L_out']))
    print(f'EDGE noise_conv C {C} stride {s} K {K} L_out 1, 2, 33, {8192 // s + 1}: uses {max(shares):.3f} of the bound')
    assert max(shares) <= 1.0


# ---- one whole generator with odd phase counts ----------------------------------------------------------------------------------------------------
ODD = dict(CONFIG, upsample_rates=[5, 3, 2], upsample_kernel_sizes=[11, 7, 4], upsample_initial_channel=64)


def _oracle64(p, h, mel):
    p64 = {k: v.double() for k, v in p.items()}
    return HO.generator(p64, h, mel.double(), None)


def test_odd_phase_generator_against_the_oracle():
    """upsample_rates [5, 3, 2] (general store path twice, then the 8-byte one), B = 2, T = 7, without the source.  Allowed: the larger of 4 x the
    oracle's own float32 error against its float64 run and RULE max|y| (the yardstick of tests/test_gpu_hifigan_train.py)."""
    h = dict(ODD, use_pitch_embed=False)
    p = HO.synth_generator_params(h, 1234)
    m = HifiGanGenerator(h)
    m.load_state_dict(p, strict=True)
    m = m.to(DEV)
    mel = torch.randn(2, 80, 7, generator=torch.Generator().manual_seed(77))
    with torch.no_grad():
        y64 = _oracle64(p, h, mel)
        y32 = HO.generator(p, h, mel, None)
    got = m(mel.to(DEV)).cpu()
    assert got.shape == y64.shape == (2, 1, 7 * 30) and bool(torch.isfinite(got).all())
    e32 = float((y32.double() - y64).abs().max())
    lim = max(4 * e32, E.RULE * float(y64.abs().max()))
    err = float((got.double() - y64).abs().max())
    print(f'EDGE generator [5, 3, 2] B 2 T 7: max err {err:.3e} <= {lim:.3e} (float32 oracle {e32:.3e}, max|y| {float(y64.abs().max()):.3f})')
    assert err <= lim


def test_odd_phase_generator_refuses_the_source_at_hop_30():
    """with f0 the module refuses a hop that is not a power of two (its f0 upsampling is index // hop): no waveform to compare - see LEFT OUT above"""
    h = dict(ODD, use_pitch_embed=True)
    m = HifiGanGenerator(h)
    m.load_state_dict(HO.synth_generator_params(h, 1235), strict=True)
    m = m.to(DEV)
    ri, nz = draws_like_reference(5, 2, 7 * 30)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 80, 7, device=DEV), torch.full((2, 7), 200.0, device=DEV), rand_ini=ri.to(DEV), noise=nz.to(DEV))


# ---- ParallelWaveGAN ------------------------------------------------------------------------------------------------------------------------------
def _pwg_layer(ops, c, L, aux, dil, first, out_fill=NAN):
    B = c['x'].shape[0]
    LS = padded_samples(L)
    w1, w2 = ops.pack(_d(c['w1'][:, :, None])), ops.pack(_d(c['w2'][:, :, None]))
    b1, b2 = _d(c['b1']), _d(c['b2'])
    xd = _d(E.cm(c['x']))
    cd = _d(E.cm(c['c'])) if aux else None
    xo = _nan(B, 64, LS)
    sk = _nan(B, 64, LS) if first else _d(E.cm(c['prev']))
    rc = ops.lib.dsv_pwg_layer(xd.data_ptr(), _p(cd), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xo.data_ptr(), sk.data_ptr(), B, L, aux, dil,
                               1 if first else 0, _stream())
    return rc, xo, sk


@pytest.mark.parametrize('aux', E.PWG_AUX)
def test_pwg_layer(aux):
    ops = _HipOps()
    shares = []
    for L in E.PWG_LENGTHS:
        for dil in E.PWG_DILATIONS:
            for first in (True, False):
                c = E.pwg_case(2, L, aux)
                rc, xo, sk = _pwg_layer(ops, c, L, aux, dil, first)
                _lib.check(rc, 'dsv_pwg_layer')
                wx, bx, ws, bs, _ = E.pwg_layer64(c['x'], c['c'], c['w1'], c['b1'], c['w2'], c['b2'], dil, prev=None if first else c['prev'])
                s = max(_share(xo, wx, bx, L), _share(sk, ws, bs, L))
                assert s <= 1.0, (aux, L, dil, first, s)
                shares.append(s)
    print(f'EDGE pwg_layer n_aux {aux} L {E.PWG_LENGTHS} dil {E.PWG_DILATIONS}: uses {max(shares):.3f} of the bound')


@pytest.mark.parametrize('L,dil,aux', [(97, 1, 80), (33, 32, 128)])
def test_pwg_layer_gate_allowance_and_saturation(L, dil, aux):
    """conv1x1_skip = identity, first = 1: the skip output IS the gate z = tanh(a) sigmoid(g), bit for bit (products by 1 and 0 in the MFMA).
    Unit-scale pre-activations, then pre-activations scaled to beyond +-100: finite, within the bound, exactly +-1 where |a| >= 20 and g >= 20,
    exactly 0 where g <= -110 (float32 holds nothing that small)."""
    ops = _HipOps()
    for scale in (1.0, 25.0):
        c = E.pwg_case(2, L, aux, scale=scale, observe_gate=True)
        rc, xo, sk = _pwg_layer(ops, c, L, aux, dil, True)
        _lib.check(rc, 'dsv_pwg_layer')
        wx, bx, ws, bs, z = E.pwg_layer64(c['x'], c['c'], c['w1'], c['b1'], c['w2'], c['b2'], dil)
        assert float((ws[:, :, :L] - z).abs().max()) <= 1e-15
        share = max(_share(xo, wx, bx, L), _share(sk, ws, bs, L))
        at, ag, _, _ = E.pwg_gate64(c['x'], c['c'], c['w1'], c['b1'], dil)
        zd = sk[:, :, :L].cpu().double()
        print(f'EDGE pwg gate L {L} dil {dil} n_aux {aux} scale {scale:g}: max|a| {float(at.abs().max()):.0f} max|g| {float(ag.abs().max()):.0f}; uses {share:.3f} '
              f'of the bound; |z - z64| {float((zd - z).abs().max()):.2e}')
        assert share <= 1.0
        if scale > 1:
            assert float(at.abs().max()) >= 100 and float(ag.abs().max()) >= 100
            hi, lo, on, off = at >= 20, at <= -20, ag >= 20, ag <= -110
            assert int((hi & on).sum()) and int((lo & on).sum()) and int(off.sum())
            assert bool((zd[hi & on] == 1.0).all()) and bool((zd[lo & on] == -1.0).all()) and bool((zd[off] == 0.0).all())


def test_pwg_gate_allowance_on_exact_preactivations():
    """The gate alone: one-hot rows in the first contraction (tanh row r = x[r](t), gate row r = x[r](t - d), no bias) make the device's
    pre-activations EXACT (products by 1 and 0), conv1x1_skip = identity shows z.  |z - tanh(a) sigmoid(g)| is then the error of the float32
    gate itself, to be inside GATE = 16 U (the derivation in tests/voc_edge_helpers.py counts 8 U); pre-activations over +-16."""
    ops = _HipOps()
    L, dil = 97, 3
    c = E.pwg_case(2, L, 0, observe_gate=True)
    c['x'] = c['x'] * 4.0
    c['w1'] = torch.zeros(128, 192)
    c['w1'][torch.arange(64), 64 + torch.arange(64)] = 1.0
    c['w1'][64 + torch.arange(64), torch.arange(64)] = 1.0
    c['b1'] = torch.zeros(128)
    rc, xo, sk = _pwg_layer(ops, c, L, 0, dil, True)
    _lib.check(rc, 'dsv_pwg_layer')
    at, ag, _, _ = E.pwg_gate64(c['x'], None, c['w1'], c['b1'], dil)
    assert torch.equal(at, c['x'].double()) and torch.equal(ag[:, :, dil:], c['x'].double()[:, :, :L - dil]) and float(ag[:, :, :dil].abs().max()) == 0
    z = torch.tanh(at) * torch.sigmoid(ag)
    zd = sk[:, :, :L].cpu().double()
    assert bool(torch.isfinite(zd).all())
    err = float((zd - z).abs().max())
    print(f'EDGE pwg gate on exact pre-activations (max|a| {float(at.abs().max()):.1f}): |z - z64| {err:.3e} = {err / E.U:.2f} U = {err / E.GATE:.3f} of the gate allowance')
    assert err <= E.GATE


def test_pwg_layer_refusals():
    ops = _HipOps()
    for aux in (4, 136):
        c = E.pwg_case(1, 33, 8)
        c['c'] = torch.zeros(1, aux, 33)
        c['w1'] = torch.zeros(128, 192 + aux)
        rc, _, _ = _pwg_layer(ops, c, 33, aux, 1, True)
        assert rc != 0 and b'aux' in ops.lib.dsd_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize('L,scale', [(1, 4), (33, 2), (33, 8), (70, 4)])
def test_pwg_upsample_and_first(L, scale):
    """L scale = 4, 66, 264 (crosses a 256-thread block), 280; dsv_pwg_first at L and at L scale"""
    ops = _HipOps()
    g = torch.Generator().manual_seed(L * 10 + scale)
    B, C = 2, 5
    x, w = torch.randn(B, C, L, generator=g), torch.randn(2 * scale + 1, generator=g)
    out = _nan(B, C, padded_samples(L * scale))
    xd, wd = _d(E.cm(x)), _d(w)
    _lib.check(ops.lib.dsv_pwg_upsample(xd.data_ptr(), wd.data_ptr(), out.data_ptr(), B * C, L, scale, _stream()), 'dsv_pwg_upsample')
    want, bound = E.pwg_upsample64(x, w, scale)
    s_up = _share(out, want, bound, L * scale)
    s_first = 0.0
    for Lf in (L, L * scale):
        z, wf, bf = torch.randn(B, Lf, generator=g), torch.randn(7, generator=g), torch.randn(7, generator=g)
        zd = torch.zeros(B, padded_samples(Lf))
        zd[:, :Lf] = z
        zd, wfd, bfd = _d(zd), _d(wf), _d(bf)
        o = _nan(B, 7, padded_samples(Lf))
        _lib.check(ops.lib.dsv_pwg_first(zd.data_ptr(), wfd.data_ptr(), bfd.data_ptr(), o.data_ptr(), B, 7, Lf, _stream()), 'dsv_pwg_first')
        want, bound = E.pwg_first64(z, wf, bf)
        s_first = max(s_first, _share(o, want, bound, Lf))
    print(f'EDGE pwg_upsample L {L} scale {scale}: uses {s_up:.3f} of the bound; pwg_first: {s_first:.3f}')
    assert s_up <= 1.0 and s_first <= 1.0
