"""The vocoder's TRAINING kernels (csrc/hifigan_train.hpp, pwg_train.hpp, voc_train_common.hpp behind hifigan_train_abi.hpp / pwg_train_abi.hpp) on the
MI355X at every tiling, slab count, clamp and split seam the C ABI admits, through ctypes only, on the case tables of
tests/voc_train_edge_helpers.py (what each table reaches is asserted on the CPU by tests/test_voc_train_edges_host.py).

Judgement: the project's rule, imported (pwg_train_helpers.RULE, U, E_GATE): element-wise |device - float64| <= RULE sum|term| (+ the E_GATE terms
where a gate is recomputed), both sides from the DEVICE'S OWN operands; exactly 0 where the bound is 0; [L, LS) of every written activation
exactly 0 - tests/test_gpu_hifigan_train.py's check(), imported.  Every output is pre-filled with NaN and must come back finite, and sits between
two guards of 64 NaN floats that must still be NaN afterwards: a store past `rows`, `N` or `LS` of a clamped or partial block lands there.  Every
workspace has exactly the length the library's sizing function returns, is pre-filled with NaN and must come back finite.  Every test prints its
measured maximum beside its bound and its largest err / bound ("share").

TABLE DGRAD   k_hgt_dgrad: all four builds (<4,4>, <2,2>, each at halo 28 and 48) with one, two and three channel slabs, last slabs that are and
              are not multiples of 8, the clamped wave pair of an odd block count, partial row blocks, asymmetric and one-sided wide padding,
              L = 1, SPAN - 1, SPAN, SPAN + 1 (wide: 35, 47, 48, 49 too), `second` form, x_saved = nullptr; dsv_hgt_conv_wgrad and
              dsv_hgt_bias_grad on the same operands.
TABLE WGRAD   k_hgt_wgrad / k_split_reduce: transposed across one and two split seams, 192 polyphase rows, 8 / 12 / 15 splits; the bits of
              dsv_pwgt_wgrad_relu at 12 splits.
TABLE ROWSUM  k_hgt_rowsum_reduce at 256, 257 and 270 partials (the second pass of its loop), L = 1024 and 1025.
TABLE UP      k_hgt_up_dgrad at k = u, odd rates, L_in = 256 / 257 / 1, with the polyphase weight gradient and the bias.
TABLE NOISE   k_hgt_noise_dhar / _wgrad at strides 6 and 15, three accumulated stages, L_out = 1 and 2.
TABLE PWG     k_pwgt_layer / _gate_bwd / _conv_bwd / _wgrad at aux 40, 64, 72, 128 and the three weight gradients at 12 splits.
WHOLE MODULE  forward_train / backward of a v3-style generator (kernel 7 at dilation 12 on 64 and 32 channels: <2,2>wide, and <4,4>wide in two
              slabs), NSF and plain; odd rates [5, 3, 2]; one frame.

DEVIATION, with the reason: the odd-rate configuration WITH the NSF source.  HifiGanGenerator.forward_train refuses a hop that is no power of two
when f0 is given, as forward does (tests/test_gpu_voc_edges.py pins that refusal): there is no gradient to compare.  The case is kept as the
refusal it is (test_module_odd_rates_refuses_the_source), the same configuration runs without the source, and the noise convolutions of that
configuration (strides 6 and 2, and 15) run at operator level in TABLE NOISE.

MEASURED on the MI355X, 2026-10-20 (all 99 cases pass in 5.4 s; NO KERNEL AND NO HOST DISPATCH WAS CHANGED: no case found a fault, a guard written, an
unwritten element or an error above its bound).  "share" = largest |device - float64| / bound over the elements of every case of the line.
  TABLE DGRAD, per instantiation over all its rows, lengths and forms (dx / dw / db):
      <4,4>      0.311 / 0.366 / 0.005          <4,4>wide  0.280 / 0.324 / 0.018
      <2,2>      0.263 / 0.306 / 0.010          <2,2>wide  0.307 / 0.402 / 0.019
  TABLE WGRAD (dw): transposed u2 k4 L = S + 1 0.165, u4 k8 L = 2 S + 37 0.177, u8 k16 at 192 rows 0.222; 8 / 12 / 15 splits 0.042 / 0.046 / 0.029;
      dsv_pwgt_wgrad_relu and dsv_hgt_conv_wgrad at 12 splits: the same bits
  TABLE ROWSUM (db; float64 sums, so the share is the one rounding of the result): 270 / 256 / 257 partials 0.009 / 0.030 / 0.031; L 1024 0.058, L 1025 0.052
  TABLE UP (dx / dw / db): u2 k2 0.138 / 0.198 / 0.004; u5 k11 0.244 / 0.127 / 0.002; u3 k7 L 257 0.237 / 0.293 / 0.003;
      u8 k16 L 256 0.248 / 0.164 / 0.001; u4 k8 L 1 0.028 / 0.079 / 0.017
  TABLE NOISE (largest of dw / db / dhar over the stages): s6 0.090; s15 + s3 + s1 accumulated 0.102; s15 L_out 1 0.072, L_out 2 0.106; s6 L_out 1 0.079
  TABLE PWG (a / da / dx / dC / dW1 / db1, the larger of first = 1, 0; dsv_pwgt_layer bitwise dsv_pwg_layer in every case):
      aux 40   0.226 / 0.432 / 0.263 / 0.331 / 0.201 / 0.031        aux 72   0.222 / 0.344 / 0.174 / 0.321 / 0.210 / 0.029
      aux 64   0.258 / 0.360 / 0.209 / 0.457 / 0.226 / 0.025        aux 128  0.244 / 0.362 / 0.261 / 0.373 / 0.186 / 0.030
      12 splits, aux 16: dW1 0.051, dW2 0.012 (last block 0.012), last_conv_layers[1] 0.044; biases <= 0.006
  two calls, one row per table (three slabs; 12 splits; 270 partials; u5 k11; three noise stages; aux 72): the same bits
  WHOLE MODULE, largest err / tolerance over the tensors (tolerances: TH.tolerances, margin 4, against float64 on the device's own masks):
      v3-style NSF 0.269 (noise_convs.0.weight), plain 0.447 (conv_pre.bias); odd rates [5, 3, 2] without the source 0.914 (resblocks.3.convs1.0.bias, at the floor
      RULE max|grad| = 2.9e-8); one frame plain 0.762, NSF 0.900 (resblocks.8.convs1.1.bias, at the floor 2.0e-8); forward_train bitwise forward() in every case
"""
import pytest
import torch

from tests import hifigan_train_helpers as TH
from tests import pwg_train_helpers as PH
from tests import voc_edge_helpers as E
from tests import voc_train_edge_helpers as V
from tests.test_gpu_hifigan_train import Ops, build, check, draws, judge, ref32_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


class EdgeOps(Ops):
    """tests/test_gpu_hifigan_train.py's Ops with guarded outputs and checked workspaces"""

    def __init__(self):
        super().__init__()
        self.outs, self.wss = [], []
        assert self.lib.dsv_pwgt_wgrad_split() == self.split

    def nan(self, *shape):
        """an output: NaN-filled, between two guards of NaN"""
        n = 1
        for s in shape:
            n *= int(s)
        raw = torch.full((n + 2 * V.GUARD,), NAN, device=DEV)
        self.outs.append((raw, n))
        return raw[V.GUARD:V.GUARD + n].view(*shape)

    def guarded(self, t):
        """a running sum the kernel adds into: its incoming value, between two guards"""
        v = self.nan(*t.shape)
        v.copy_(t)
        return v

    def ws(self, n, f64=False):
        """a workspace of exactly n floats (the library's sizing function's answer), NaN-filled"""
        assert n > 0, 'the sizing function refused the shape'
        t = torch.full((n,), NAN, device=DEV)
        self.wss.append((t, f64))
        return t

    def wgrad(self, g, x, B, Co, Ci, K, pad, dil, L, up, slope):
        n = self.lib.dsv_hgt_wgrad_workspace_floats(B, L, Co, Ci, K, up)
        ws, dw = self.ws(n), self.nan(Co * up, K, Ci)
        self.call('dsv_hgt_conv_wgrad', g.data_ptr(), x.data_ptr(), ws.data_ptr(), n, dw.data_ptr(), B, Co, Ci, K, pad, dil, L, up, slope)
        return dw

    def bias(self, g, B, C, L):
        n = self.lib.dsv_hgt_bias_workspace_floats(B, C, L)
        ws, db = self.ws(n, f64=True), self.nan(C)
        self.call('dsv_hgt_bias_grad', g.data_ptr(), ws.data_ptr(), n, db.data_ptr(), B, C, L)
        return db

    def pwg_ws(self, B, L, n):
        return self.ws(self.lib.dsv_pwgt_wgrad_workspace_floats(B, L, n))

    def pack2(self, mat):
        return self.pack(mat[:, :, None])

    def finish(self):
        outs, wss = self.outs, self.wss
        self.outs, self.wss = [], []
        for raw, n in outs:
            assert bool(torch.isnan(raw[:V.GUARD]).all()) and bool(torch.isnan(raw[V.GUARD + n:]).all()), 'a guard was written'
            assert bool(torch.isfinite(raw[V.GUARD:V.GUARD + n]).all()), 'an output element was not written'
        for t, f64 in wss:
            assert bool(torch.isfinite(t.view(torch.float64) if f64 else t).all()), 'a workspace element was not written'


@pytest.fixture(scope='module')
def edge_ops():
    return EdgeOps()


@pytest.fixture
def ops(edge_ops):
    edge_ops.outs, edge_ops.wss = [], []
    yield edge_ops
    edge_ops.finish()


def share(name, got, want, bound, L=None):
    """the existing check(), then err / bound"""
    check(name, got, want, bound, L)
    g = TH.d64(got)
    return E.used(g if L is None else g[..., :L], want, bound)


def report(table, what, shares):
    print(f'EDGE {table} | {what} | ' + ' '.join(f'{k}={v:.3f}' for k, v in shares.items()))
    assert max(shares.values()) <= 1.0


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f'{k}: two calls differ'


# ---- TABLE DGRAD ----------------------------------------------------------------------------------------------------------------------------------
def run_dgrad(ops, case):
    tag, C, Cg, K, dil, pad, B, L, form, masked = case
    o = V.dgrad_operands(case)
    t = dict(g=ops.padded(o['g']), x=ops.padded(o['x']), res=None if o['res'] is None else ops.padded(o['res']),
             sum_in=None if o['sum_in'] is None else ops.padded(o['sum_in']), w=o['w'])
    dx = ops.nan(B, C, ops.ls(L))
    ops.call('dsv_hgt_conv_dgrad', t['g'].data_ptr(), ops.pack(o['w'].flip(2).transpose(0, 1)).data_ptr(), t['x'].data_ptr() if masked else None,
             ops.p(t['res']), ops.p(t['sum_in']), dx.data_ptr(), B, Cg, C, K, pad, dil, L, V.SLOPE, o['divide'])
    dw = ops.wgrad(t['g'], t['x'], B, Cg, C, K, pad, dil, L, 1, V.SLOPE)
    return dict(dx=dx, dw=dw, db=ops.bias(t['g'], B, Cg, L)), t


@pytest.mark.parametrize('case', V.dgrad_cases(), ids=V.dgrad_id)
def test_table_dgrad(ops, case):
    tag, C, Cg, K, dil, pad, B, L, form, masked = case
    assert V.dgrad_dispatch(C, Cg, K, dil, pad)['tag'] == tag
    out, t = run_dgrad(ops, case)
    ref = V.dgrad_reference(case, V.cut(t['g'], L), t['w'].double(), V.cut(t['x'], L), V.cut(t['res'], L), V.cut(t['sum_in'], L))
    report('DGRAD', V.dgrad_id(case), dict(dx=share('dx', out['dx'], *ref['dx'], L), dw=share('dw', out['dw'].permute(0, 2, 1), *ref['dw']),
                                           db=share('db', out['db'], *ref['db'])))


# ---- TABLE WGRAD ----------------------------------------------------------------------------------------------------------------------------------
def run_wgrad(ops, kind, i):
    c = V.wgrad_operands(kind, i, ops.split)
    g, x = ops.padded(c['g']), ops.padded(c['x'])
    if kind == 'up':
        r, t, kk, ppad = V.taps_of(c['k'], c['u'])
        dwp = ops.wgrad(g, x, c['B'], c['Co'], c['Ci'], kk, ppad, 1, c['L'], c['u'], V.SLOPE).view(c['Co'], c['u'], kk, c['Ci'])
        dw = dwp[:, torch.tensor(r, device=DEV), torch.tensor(t, device=DEV), :].permute(2, 0, 1)
        # the columns of the polyphase filter no tap sits in multiply samples too, and no plain weight reads them: finite is all they owe
    else:
        dw = ops.wgrad(g, x, c['B'], c['Co'], c['Ci'], c['k'], 1, 1, c['L'], 1, V.SLOPE).permute(0, 2, 1)
    return dict(dw=dw), c, g, x


@pytest.mark.parametrize('kind,i', V.wgrad_cases())
def test_table_wgrad(ops, kind, i):
    out, c, g, x = run_wgrad(ops, kind, i)
    want, bound = V.wgrad_reference(c, V.cut(g, c['L'] * c['u']), V.cut(x, c['L']))
    splits = V.splits_of(c['B'], c['L'], ops.split)
    report('WGRAD', f'{kind} B{c["B"]} Ci{c["Ci"]} Co{c["Co"]} u{c["u"]} k{c["k"]} L{c["L"]} ({splits} splits)', dict(dw=share('dw', out['dw'], want, bound)))


def test_both_weight_gradients_return_the_same_bits_at_twelve_splits(ops):
    """tests/test_gpu_hifigan_train.py's guard (dsv_pwgt_wgrad_relu rows 0..63 and dsv_hgt_conv_wgrad at Co = Ci = 64, K = 1, slope 0 state the
    same sum on the same splits) at B 3, L = 3 S + 5: k_split_reduce's unrolled body and its remainder"""
    B, C, L = V.WGRAD_BITS
    L = V.length(L, ops.split)
    assert V.splits_of(B, L, ops.split) == 12 and C == 64
    g, saved = ops.padded(V.rnd(B, C, L, seed=7 * L + 1)), ops.padded(V.rnd(B, C, L, seed=7 * L + 2))
    assert 0.3 < float((saved[..., :L] < 0).float().mean()) < 0.7
    out = ops.nan(128 * 64 + 128)
    ops.call('dsv_pwgt_wgrad_relu', g.data_ptr(), saved.data_ptr(), ops.pwg_ws(B, L, 64).data_ptr(), out.data_ptr(), B, L)
    dw = ops.wgrad(g, saved, B, 64, 64, 1, 0, 1, L, 1, 0.0).reshape(64, 64)
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0
    assert torch.equal(out[:64 * 64].reshape(64, 64), dw)


# ---- TABLE ROWSUM ---------------------------------------------------------------------------------------------------------------------------------
def run_rowsum(ops, case):
    B, C, L = case
    g = ops.padded(V.rowsum_operand(B, C, L))
    return dict(db=ops.bias(g, B, C, L)), g


@pytest.mark.parametrize('B,C,L', V.ROWSUM)
def test_table_rowsum(ops, B, C, L):
    out, g = run_rowsum(ops, (B, C, L))
    report('ROWSUM', f'B{B} C{C} L{L} ({V.partials_of(B, L)} partials)', dict(db=share('db', out['db'], *V.rowsum_reference(V.cut(g, L)))))


# ---- TABLE UP -------------------------------------------------------------------------------------------------------------------------------------
def run_up(ops, case):
    B, Ci, Co, u, k, L, div = case
    o = V.up_operands(case)
    g, x = ops.padded(o['g']), ops.padded(o['x'])
    dx = ops.nan(B, Ci, ops.ls(L))
    ops.call('dsv_hgt_upsample_dgrad', g.data_ptr(), o['w'].to(DEV).contiguous().data_ptr(), x.data_ptr(), dx.data_ptr(), B, Ci, Co, u, k, L, V.SLOPE, div)
    r, t, kk, ppad = V.taps_of(k, u)
    dwp = ops.wgrad(g, x, B, Co, Ci, kk, ppad, 1, L, u, V.SLOPE).view(Co, u, kk, Ci)
    dw = dwp[:, torch.tensor(r, device=DEV), torch.tensor(t, device=DEV), :].permute(2, 0, 1)
    return dict(dx=dx, dw=dw, db=ops.bias(g, B, Co, L * u)), g, x, o['w']


@pytest.mark.parametrize('case', V.UP, ids=lambda c: f'B{c[0]}-Ci{c[1]}-Co{c[2]}-u{c[3]}k{c[4]}-L{c[5]}-div{c[6]:g}')
def test_table_up(ops, case):
    B, Ci, Co, u, k, L, div = case
    out, g, x, w = run_up(ops, case)
    ref = V.up_reference(case, V.cut(g, L * u), V.cut(x, L), w.double())
    report('UP', f'u{u} k{k} Ci{Ci} Co{Co} B{B} L{L}', dict(dx=share('dx', out['dx'], *ref['dx'], L), dw=share('dw', out['dw'], *ref['dw']),
                                                           db=share('db', out['db'], *ref['db'])))


# ---- TABLE NOISE ----------------------------------------------------------------------------------------------------------------------------------
def run_noise(ops, Lh, stages, judged=None):
    """dhar is accumulated over the stages in call order; its bound is the sum of the stages' bounds (tests/test_gpu_hifigan_train.py)"""
    B = V.NOISE_B
    har0, st = V.noise_operands(Lh, stages)
    har = ops.padded(har0)
    dhar = ops.nan(B, ops.ls(Lh))
    out = {}
    want_h, bound_h = 0.0, 0.0
    for n, s in enumerate(st):
        g = ops.padded(s['g'])
        dw, db = ops.nan(s['C'], s['K']), ops.nan(s['C'])
        nws = ops.lib.dsv_hgt_bias_workspace_floats(B, s['C'], s['Lo'])
        ws = ops.ws(nws, f64=True)
        ops.call('dsv_hgt_noise_conv_backward', g.data_ptr(), har.data_ptr(), s['w'].to(DEV).contiguous().data_ptr(), ws.data_ptr(), nws, dw.data_ptr(),
                 db.data_ptr(), dhar.data_ptr(), B, s['C'], s['K'], s['s'], s['pad'], Lh, s['Lo'], 1 if n == 0 else 0)
        out[f'dw{n}'], out[f'db{n}'] = dw, db
        if judged is not None:
            (ww, bw), (wb, bb), (wh, bh) = TH.noise_conv_backward(V.cut(g, s['Lo']), V.cut(har, Lh), s['w'].double(), s['s'], s['pad'])
            want_h, bound_h = want_h + wh, bound_h + bh
            judged[f'dw{n}'], judged[f'db{n}'] = share(f'dw{n}', dw, ww, bw), share(f'db{n}', db, wb, bb)
            judged[f'dhar{n}'] = share(f'dhar after stage {n}', dhar, want_h, bound_h, Lh)
    out['dhar'] = dhar
    return out


@pytest.mark.parametrize('Lh,stages', V.NOISE, ids=lambda v: str(v).replace(' ', ''))
def test_table_noise(ops, Lh, stages):
    judged = {}
    run_noise(ops, Lh, stages, judged)
    louts = [V.noise_geometry(Lh, s, K)[1] for _, s, K in stages]
    report('NOISE', f'Lh{Lh} {stages} L_out {louts}', judged)


# ---- TABLE PWG ------------------------------------------------------------------------------------------------------------------------------------
def run_pwg_block(ops, aux, first, judged=None):
    B, L, dil = V.PWG_BLOCK
    o = V.pwg_operands(aux, B, L)
    w = o['w']
    LS = ops.ls(L)
    x, c, prev = ops.padded(o['x']), ops.padded(o['c']), ops.padded(o['prev'])
    w1 = ops.pack2(torch.cat([w['wc'].permute(0, 2, 1).reshape(128, 192), w['wa'][:, :, 0]], 1))
    w2 = ops.pack2(torch.cat([w['wo'][:, :, 0], w['ws'][:, :, 0]], 0))
    b1, b2 = w['bc'].to(DEV), torch.cat([w['bo'], w['bs']]).to(DEV)
    # the training forward against the inference layer, and its saved pre-activations
    xo, sk = ops.nan(B, 64, LS), (ops.nan(B, 64, LS) if first else ops.guarded(prev))
    ops.call('dsv_pwg_layer', x.data_ptr(), c.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xo.data_ptr(), sk.data_ptr(), B, L, aux,
             dil, first)
    xt, st, at = ops.nan(B, 64, LS), (ops.nan(B, 64, LS) if first else ops.guarded(prev)), ops.nan(B, 128, LS)
    ops.call('dsv_pwgt_layer', x.data_ptr(), c.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xt.data_ptr(), st.data_ptr(),
             at.data_ptr(), B, L, aux, dil, first)
    assert torch.equal(xo, xt) and torch.equal(sk, st), 'dsv_pwgt_layer is not bitwise dsv_pwg_layer'
    # gate backward on drawn pre-activations, then the convolution's data backward with the conditioning gradient
    dxp, dS, a = ops.padded(o['dxp']), ops.padded(o['dS']), ops.padded(o['a'])
    assert float(a.abs().max()) <= V.GATE_RANGE                                 # the range E_GATE was computed over
    da = ops.nan(B, 128, LS)
    ops.call('dsv_pwgt_gate_backward', dxp.data_ptr(), dS.data_ptr(), a.data_ptr(),
             ops.pack2(torch.cat([w['ws'][:, :, 0].t(), w['wo'][:, :, 0].t()], 1)).data_ptr(), da.data_ptr(), B, L)
    R = (aux + 31) // 32 * 32
    wat = ops.pack2(torch.nn.functional.pad(w['wa'][:, :, 0].t(), (0, 0, 0, R - aux)))
    dcp = ops.padded(o['dc_prev'])
    dc = ops.nan(B, aux, LS) if first else ops.guarded(dcp)
    dx = ops.nan(B, 64, LS)
    ops.call('dsv_pwgt_conv_backward', da.data_ptr(), dxp.data_ptr(), ops.pack2(w['wc'].permute(1, 2, 0).reshape(64, 384)).data_ptr(), wat.data_ptr(),
             dx.data_ptr(), dc.data_ptr(), B, L, aux, dil, first)
    n1 = 192 + aux
    dw1 = ops.nan(128 * n1 + 128)
    ops.call('dsv_pwgt_wgrad_conv', da.data_ptr(), x.data_ptr(), c.data_ptr(), ops.pwg_ws(B, L, n1).data_ptr(), dw1.data_ptr(), B, L, aux, dil)
    if judged is not None:
        d = lambda t: V.cut(t, L)                                               # noqa: E731
        judged['a'] = share('a', at, *V.pwg_forward_reference(w, d(x), d(c), dil), L)
        judged['da'] = share('da', da, *PH.gate_backward(d(dxp), d(dS), d(a), w['wo'].double(), w['ws'].double()), L)
        (wx, bx), (wc_, bc_) = PH.conv_backward(d(da), d(dxp), w['wc'].double(), w['wa'].double(), dil, None if first else d(dcp))
        judged['dx'], judged['dC'] = share('dx', dx, wx, bx, L), share('dC', dc, wc_, bc_, L)
        (dw, bw), (db, bb) = PH.wgrad_conv(d(da), d(x), d(c), dil)
        judged['dW1'], judged['db1'] = share('dW1', dw1[:128 * n1].reshape(128, n1), dw, bw), share('db1', dw1[128 * n1:], db, bb)
    return dict(xt=xt, st=st, at=at, da=da, dx=dx, dc=dc, dw1=dw1)


@pytest.mark.parametrize('aux,first', V.pwg_cases())
def test_table_pwg_blocks(ops, aux, first):
    judged = {}
    run_pwg_block(ops, aux, first, judged)
    report('PWG', f'aux {aux} first {first}', judged)


def test_table_pwg_weight_gradients_at_twelve_splits(ops):
    aux, B, L = V.PWG_SPLITS
    L = V.length(L, ops.split)
    assert V.splits_of(B, L, ops.split) == 12
    dil, n1 = 1, 192 + aux
    o = V.pwg_operands(aux, B, L)
    d = lambda t: V.cut(t, L)                                                   # noqa: E731
    da, x, c = ops.padded(V.rnd(B, 128, L, seed=L + 7)), ops.padded(o['x']), ops.padded(o['c'])
    out = ops.nan(128 * n1 + 128)
    ops.call('dsv_pwgt_wgrad_conv', da.data_ptr(), x.data_ptr(), c.data_ptr(), ops.pwg_ws(B, L, n1).data_ptr(), out.data_ptr(), B, L, aux, dil)
    (dw, bw), (db, bb) = PH.wgrad_conv(d(da), d(x), d(c), dil)
    judged = dict(dW1=share('dW1', out[:128 * n1].reshape(128, n1), dw, bw), db1=share('db1', out[128 * n1:], db, bb))
    dxp, dS, a = ops.padded(o['dxp']), ops.padded(o['dS']), ops.padded(o['a'])
    assert float(a.abs().max()) <= V.GATE_RANGE
    for name, dx_ in (('dW2', dxp), ('dW2last', None)):
        out2 = ops.nan(128 * 64 + 128)
        ops.call('dsv_pwgt_wgrad_out', ops.p(dx_), dS.data_ptr(), a.data_ptr(), ops.pwg_ws(B, L, 64).data_ptr(), out2.data_ptr(), B, L)
        (dw, bw), (db, bb) = PH.wgrad_out(None if dx_ is None else d(dx_), d(dS), d(a))
        judged[name], judged[name + 'b'] = share(name, out2[:128 * 64].reshape(128, 64), dw, bw), share(name + ' bias', out2[128 * 64:], db, bb)
    g, saved = ops.padded(o['g']), ops.padded(o['saved'])
    out3 = ops.nan(128 * 64 + 128)
    ops.call('dsv_pwgt_wgrad_relu', g.data_ptr(), saved.data_ptr(), ops.pwg_ws(B, L, 64).data_ptr(), out3.data_ptr(), B, L)
    (dw, bw), (db, bb) = PH.wgrad_relu(d(g), d(saved))
    judged['dWrelu'], judged['dbrelu'] = share('dW last1', out3[:64 * 64].reshape(64, 64), dw, bw), share('db last1', out3[128 * 64:128 * 64 + 64], db, bb)
    assert float(out3[64 * 64:128 * 64].abs().max()) == 0.0 and float(out3[128 * 64 + 64:].abs().max()) == 0.0
    report('PWG', f'weight gradients aux {aux} B{B} L{L} (12 splits)', judged)


# ---- two calls return equal bits: one row per table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table', ['DGRAD', 'WGRAD', 'ROWSUM', 'UP', 'NOISE', 'PWG'])
def test_two_calls_return_the_same_bits(ops, table):
    """"No atomics; every sum runs in a fixed order" on the multi-slab, multi-split and multi-partial paths"""
    run = {'DGRAD': lambda: run_dgrad(ops, V.DGRAD_REPEAT)[0], 'WGRAD': lambda: run_wgrad(ops, *V.WGRAD_REPEAT)[0],
           'ROWSUM': lambda: run_rowsum(ops, V.ROWSUM[V.ROWSUM_REPEAT])[0], 'UP': lambda: run_up(ops, V.UP[V.UP_REPEAT])[0],
           'NOISE': lambda: run_noise(ops, *V.NOISE[V.NOISE_REPEAT]), 'PWG': lambda: run_pwg_block(ops, *V.PWG_REPEAT)}[table]
    same_bits(run(), run())


# ---- the whole module -----------------------------------------------------------------------------------------------------------------------------
def _f0(B, T, seed):
    f0 = 200.0 + 80.0 * torch.rand(B, T, generator=torch.Generator().manual_seed(seed))
    if T > 2:
        f0[B - 1, 1:3] = 0.0                                                    # an unvoiced stretch
    return f0


@pytest.mark.parametrize('nsf', [True, False], ids=['nsf', 'plain'])
def test_module_v3_style(nsf):
    """resblock '2', kernels [3, 5, 7], dilations [[1, 2], [2, 6], [3, 12]], c0 128, rates [8, 8, 4], B 2, 4 frames = 1024 samples: kernel 7 at
    dilation 12 reaches 36 samples - <2,2>wide on the 64-channel stage, <4,4>wide in two slabs (24 + 8) on the 32-channel stage"""
    h = TH.config(use_pitch_embed=nsf, **V.V3)
    B, T = 2, 4
    Ls = T * TH.hop_of(h)
    assert Ls == 1024
    state = TH.synth_state(TH.module_shapes(h), 81)
    x, target = V.rnd(B, 80, T, seed=82), V.rnd(B, 1, Ls, seed=83, scale=0.5)
    f0, dr = (_f0(B, T, 84), draws(85, B, Ls)) if nsf else (None, None)
    loss = TH.mse_to(target)
    judge(f'v3 {"nsf" if nsf else "plain"}', build(h, state), h, x, f0, dr, loss, ref32_err(h, x, f0, loss))


def test_module_odd_rates():
    """rates [5, 3, 2], kernels [11, 7, 4], c0 64, B 1, 3 frames = 90 samples, without the source (see DEVIATION above)"""
    h = TH.config(**V.ODD)
    state = TH.synth_state(TH.module_shapes(h), 91)
    x, target = V.rnd(1, 80, 3, seed=92), V.rnd(1, 1, 90, seed=93, scale=0.5)
    loss = TH.mse_to(target)
    judge('odd rates', build(h, state), h, x, None, None, loss, ref32_err(h, x, None, loss))


def test_module_odd_rates_refuses_the_source():
    """the odd-rate configuration as NSF, B 1, 3 frames: forward_train refuses a hop of 30 when f0 is given, with forward()'s message"""
    h = TH.config(use_pitch_embed=True, **V.ODD)
    m = build(h, TH.synth_state(TH.module_shapes(h), 94))
    ri, nz = draws(95, 1, 90)
    with pytest.raises(NotImplementedError, match='power-of-two hop sizes only'):
        m.forward_train(V.rnd(1, 80, 3, seed=96).to(DEV), _f0(1, 3, 97).to(DEV), rand_ini=ri, noise=nz)


@pytest.mark.parametrize('case', TH.CASES)
def test_module_one_frame(case):
    """the fixture configuration and state at B 1, T = 1: 64 samples, every stage shorter than one tile"""
    fx = TH.fixture(case)
    h = fx['h']
    x, target = V.rnd(1, 80, 1, seed=101), V.rnd(1, 1, TH.hop_of(h), seed=102, scale=0.5)
    f0, dr = (torch.full((1, 1), 220.0), draws(103, 1, TH.hop_of(h))) if case == 'nsf' else (None, None)
    loss = TH.mse_to(target)
    judge(f'one frame {case}', build(h, fx['state']), h, x, f0, dr, loss, ref32_err(h, x, f0, loss), fx['none_keys'])
