"""The FastSpeech2 training objective (csrc/fs2_loss.hpp: k_mel_loss_fwd / _final / _bwd, k_dur_loss_rows<false|true> / _final) on the MI355X at
its tiles, seams and limits, through the C ABI with ctypes (dsf_mel_loss, dsf_mel_loss_bwd, dsf_dur_loss, dsf_dur_loss_bwd) on the case tables
of tests/fs2_loss_edge_helpers.py, and through diffsinger_amd/losses.py on the strided cwt view (what each table reaches is asserted on the CPU
by tests/test_fs2_loss_edges_host.py, which also shows that the yardstick catches six restated faults).

Judgement: tests/test_gpu_fs2_loss.py's rule and floors - the device's distance from float64 <= max(2 x the CPU fp32 restatement's own distance
from float64, floor), floors 1e-5 (mel values, map), 2e-7 (mel gradient), 1e-6 (duration values and gradient) - applied PER ROW to the map and
the gradients (fs2_loss_edge_helpers.row_ratio): a seam frame cannot hide behind the bulk.  out[3], the weight count, is compared exactly;
integer durations are compared exactly through pdur at dur_pred = log(dur_gt + 1), which must be exactly 0.  Every input, output and workspace
lies between two guards of 64 NaN floats, the gaps a strided layout leaves between rows are NaN too, and after the calls every guard, gap and
input must hold the bits it held before.  Outputs and workspaces are NaN-filled before a call and finite afterwards (of the duration workspace:
the six row sums and three totals the header names), except on the `bad` path, where the three losses and every gradient must be NaN.  Every
call is made twice and the second must return the first one's bits.  Every test prints the device's distance beside its allowance.

NOT ASSERTED, by design: the all-zero-target BATCH (0 / 0: the kernel's gradient is 0 where torch's is NaN; it is rejected from the table), and
wdur under silence ids with a single phone (no kept word can exist: 0 / 0 on the device and in torch alike; pdur, sdur and their gradient are
compared with grad_out[1] = 0).

WHAT THE FIRST RUN FOUND, AND THE FIX.  On the fp32 kernels no case found a fault, a written guard, gap or input, an unwritten element or a
second call with other bits, but 31 of the 151 cases missed the yardstick: the SSIM map and dx by up to 2.05 in rows whose window lies in frames
where target and prediction are both zero (x + bias = y + bias: sigma = E - mu^2 cancels against 36) and at M = 1, sdur by up to 6.5 and wdur by
up to 11.4 ((log(S + 1) - log(S_gt + 1))^2 of sums a few percent apart: one ulp of logf is 1e-5 of the loss), none of them at a seam.  The
kernels now do their arithmetic in float64 on the fp32 operands (csrc/fs2_loss.hpp: k_mel_loss_fwd / _bwd sum the 11 x 11 window directly,
k_dur_loss_rows uses double exp / log and sums; pdur's target alone stays logf, see the header), at 0.27 instead of 0.18 ms for the
objective's forward + backward at 8 x 1024 x 80 (tools/bench_fs2_loss.py).

MEASURED on the MI355X, 2026-10-21, float64 kernels: all 151 cases pass in 3.6 s.  ratio = the device's distance / its allowance, worst over
every case of the family (passes at <= 1):
    MEL     out[0] 0.008   out[1] 0.013   out[2] 0.011   map 0.006   dx 0.257         (49 cases)
    CROSS   out[0..2] <= 0.009            map 0.004      dx 0.369                     (36 cases + the refusal)
    DUR     pdur 0.373     wdur 0.164     sdur 0.129     grad 0.754                   (55 cases + 3 on the bad path; 4 exact-duration cases)
    LOSSES  values <= 0.042  map 0.003  dx 0.006  d mel_out 0.070  d cwt 0.683  d dur 0.087      (3 cases)
"""
import pytest
import torch

from diffsinger_amd import _lib, losses
from tests import fs2_loss_edge_helpers as V
from tests import fs2_loss_helpers as LH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
F64, F32 = torch.float64, torch.float32


def _bits(t):
    return t.view(torch.int32)


class Harness:
    """guarded device buffers: inputs (and the gaps of their layouts) must come back unchanged, outputs written and finite, guards NaN"""

    def __init__(self):
        self.lib = _lib.load()
        self.inputs, self.outputs = [], []

    def _raw(self, floats):
        return torch.full((floats + 2 * V.GUARD,), NAN, device=DEV)

    def place(self, t, layout='contig'):
        """a CPU tensor (fp32, or int64 as pairs of floats) on the device in a layout: -> the view the kernel is given"""
        t = t.contiguous()
        if t.dtype == torch.int64:
            raw = self._raw(2 * t.numel())
            view = raw[V.GUARD:V.GUARD + 2 * t.numel()].view(torch.int64).view(t.shape)
        else:
            shape = tuple(t.shape)
            if layout != 'contig':
                B, T, M = t.shape
                shape = (B, T, M + 1) if layout == 'cwt' else (B, T + 3, M)
            n = 1
            for s in shape:
                n *= int(s)
            raw = self._raw(n)
            view = raw[V.GUARD:V.GUARD + n].view(*shape)
            if layout == 'cwt':
                view = view[:, :, :M]
            elif layout == 'rows':
                view = view[:, 2:T + 2]
        view.copy_(t)
        self.inputs.append((raw, raw.clone()))
        return view

    def out(self, *shape, owed=None):
        """an output or workspace: NaN-filled; every element (or the elements `owed`, indices into it) must come back finite"""
        n = 1
        for s in shape:
            n *= int(s)
        raw = self._raw(n)
        self.outputs.append((raw, n, owed))
        return raw[V.GUARD:V.GUARD + n].view(*shape)

    def call(self, name, *args):
        _lib.call(name, torch.device(DEV), *args)

    def finish(self, nan_ok=False):
        torch.cuda.synchronize()
        inputs, outputs = self.inputs, self.outputs
        self.inputs, self.outputs = [], []
        for raw, before in inputs:
            assert torch.equal(_bits(raw), _bits(before)), 'an input, a gap of its layout or its guard was written'
        for raw, n, owed in outputs:
            assert bool(torch.isnan(raw[:V.GUARD]).all()) and bool(torch.isnan(raw[V.GUARD + n:]).all()), 'a guard was written'
            mid = raw[V.GUARD:V.GUARD + n]
            if owed is not None:
                assert bool(torch.isfinite(mid[owed]).all()), 'a workspace element was not written'
            elif not nan_ok:
                assert bool(torch.isfinite(mid).all()), 'an output element was not written'


@pytest.fixture(scope='module')
def harness():
    return Harness()


@pytest.fixture
def h(harness):
    harness.inputs, harness.outputs = [], []
    return harness


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), f'{k}: two calls differ'


def report(family, what, ratios):
    print(f'EDGE {family} | {what} | ' + ' '.join(f'{k}={r:.3f} ({e:.1e}/{a:.1e})' for k, (r, e, a) in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v[0] <= 1.0}
    assert not bad, bad


# ---- the mel terms ----------------------------------------------------------------------------------------------------------------------
X_LAYOUT = {'contig': ('contig', 'contig'), 'cwt': ('cwt', 'cwt'), 'rows': ('rows', 'rows'), 'mixed': ('cwt', 'rows'), 'mixed_rev': ('rows', 'cwt')}


def run_mel(h, x, y, layout, bias, terms, weighted, lam, gout, R, want_map):
    """dsf_mel_loss, then dsf_mel_loss_bwd on its out[4] -> dict(out, map, dx)"""
    B, T, M = x.shape
    lx, ly = X_LAYOUT[layout]
    xd, yd = h.place(x, lx), h.place(y, ly)
    assert xd.stride(2) == 1 and yd.stride(2) == 1
    n_ws = h.lib.dsf_fs2_loss_workspace_floats(B, T, 0)
    assert n_ws == B * V.tiles(T) * 4
    ws, out = h.out(n_ws), h.out(4)
    smap = h.out(B, T, M) if want_map else None
    h.call('dsf_mel_loss', xd.data_ptr(), xd.stride(0), xd.stride(1), yd.data_ptr(), yd.stride(0), yd.stride(1), B, T, M, bias, weighted, terms,
           lam[0], lam[1], _lib.ptr(smap), ws.data_ptr(), out.data_ptr())
    g = h.place(torch.tensor(gout, dtype=F32))
    gm = h.place(R) if R is not None else None
    dx = h.out(B, T, M)
    h.call('dsf_mel_loss_bwd', xd.data_ptr(), xd.stride(0), xd.stride(1), yd.data_ptr(), yd.stride(0), yd.stride(1), B, T, M, bias, weighted, terms,
           lam[0], lam[1], out.data_ptr(), g.data_ptr(), _lib.ptr(gm), dx.data_ptr())
    return dict(out=out, map=smap, dx=dx)


def judge_mel(got, r64, r32):
    """-> {name: (ratio, distance, allowance)}; out[3] exactly"""
    assert float(got['out'][3]) == float(r64['out'][3]), 'the weight count'
    res = {f'out{i}': V.value_ratio(got['out'][i], r64['out'][i], r32['out'][i], V.FLOOR_MEL_VALUE) for i in range(3)}
    if got['map'] is not None:
        r, _, e, a = V.row_ratio(got['map'], r64['map'], r32['map'], V.FLOOR_MEL_VALUE)
        res['map'] = (r, e, a)
    r, _, e, a = V.row_ratio(got['dx'], r64['dx'], r32['dx'], V.FLOOR_MEL_GRAD)
    res['dx'] = (r, e, a)
    return res


@pytest.mark.parametrize('c', V.mel_cases(), ids=V.mel_id)
def test_table_mel(h, c):
    """terms = 3, weighted, the map, grad_out (1, 1, 0.25) and a grad_map"""
    x, y = V.mel_operands(c)
    args = (x, y, c.layout, c.bias, 3, 1, V.MEL_LAM, V.MEL_GOUT, V.mel_grad_map(c), True)
    got = run_mel(h, *args)
    same_bits(got, run_mel(h, *args))
    h.finish()
    report('MEL', V.mel_id(c), judge_mel(got, V.mel_case_reference(c, F64), V.mel_case_reference(c, F32)))


CROSS_SHAPES = (V.MelCase(3, 33, 80, 6.0, 'tail', 'contig'), V.MelCase(1, 17, 128, 6.0, 'z16', 'contig'))
CROSS = [(c, terms, weighted, want_map, gmap) for c in CROSS_SHAPES for terms in (1, 2, 3) for weighted in (0, 1)
         for want_map in ((0, 1) if terms & 2 else (0,)) for gmap in ((0, 1) if terms & 2 else (0,))]


@pytest.mark.parametrize('c,terms,weighted,want_map,gmap', CROSS, ids=lambda v: V.mel_id(v) if isinstance(v, tuple) else str(v))
def test_mel_term_combinations(h, c, terms, weighted, want_map, gmap):
    """terms {1, 2, 3} x weighted {0, 1} x map x grad_map at T = 33, M = 80 and T = 17, M = kMlMaxM, with a random grad_out"""
    x, y = V.mel_operands(c)
    gout = [float(v) for v in torch.randn(3, generator=V.gen(terms, weighted, want_map, gmap))]
    lam, R = (0.7, 1.3), V.mel_grad_map(c) if gmap else None
    args = (x, y, c.layout, c.bias, terms, weighted, lam, gout, R, bool(want_map))
    got = run_mel(h, *args)
    same_bits(got, run_mel(h, *args))
    h.finish()
    r64, r32 = (V.mel_reference(x, y, c.bias, terms, weighted, lam, gout, R, dt) for dt in (F64, F32))
    if not want_map:
        r64['map'] = r32['map'] = None
    report('CROSS', f'{V.mel_id(c)} terms {terms} weighted {weighted} map {want_map} grad_map {gmap}', judge_mel(got, r64, r32))


def test_a_map_without_the_ssim_term_is_refused(h):
    c = CROSS_SHAPES[0]
    x, y = V.mel_operands(c)
    B, T, M = x.shape
    xd, yd = h.place(x), h.place(y)
    ws, out, smap, dx = h.out(h.lib.dsf_fs2_loss_workspace_floats(B, T, 0)), h.out(4), h.out(B, T, M), h.out(B, T, M)
    g, gm = h.place(torch.ones(3)), h.place(V.mel_grad_map(c))
    s = torch.cuda.current_stream().cuda_stream
    with torch.cuda.device(DEV):
        assert h.lib.dsf_mel_loss(xd.data_ptr(), xd.stride(0), xd.stride(1), yd.data_ptr(), yd.stride(0), yd.stride(1), B, T, M, 6.0, 1, 1, 1.0, 1.0,
                                  smap.data_ptr(), ws.data_ptr(), out.data_ptr(), s) != 0
        assert b'without the SSIM term' in h.lib.dsd_last_error()
        assert h.lib.dsf_mel_loss_bwd(xd.data_ptr(), xd.stride(0), xd.stride(1), yd.data_ptr(), yd.stride(0), yd.stride(1), B, T, M, 6.0, 1, 1, 1.0, 1.0,
                                      out.data_ptr(), g.data_ptr(), gm.data_ptr(), dx.data_ptr(), s) != 0
        assert b'without the SSIM term' in h.lib.dsd_last_error()
    torch.cuda.synchronize()
    for t in (ws, out, smap, dx):
        assert bool(torch.isnan(t).all()), 'a refused call wrote'
    h.finish(nan_ok=True)


# ---- the duration terms -----------------------------------------------------------------------------------------------------------------
def run_dur(h, o, gout, lam):
    """dsf_dur_loss, then dsf_dur_loss_bwd on its workspace -> dict(out [3], grad [B,Tt], ws)"""
    B, Tt = o['tok'].shape
    T = o['mel2ph'].shape[1]
    d, m2p, tok = h.place(o['dur_pred']), h.place(o['mel2ph']), h.place(o['tok'])
    sil = h.place(torch.tensor(o['sil'], dtype=torch.int64)) if o['sil'] is not None else None
    wdb = h.place(o['wdb']) if o['wdb'] is not None else None
    n_ws = h.lib.dsf_fs2_loss_workspace_floats(B, Tt, 1)
    assert n_ws == B * 8 + 8
    # the workspace holds 6 of 8 floats per row and 3 totals (csrc/fs2_loss.hpp, kDurRow): those are owed, the rest stays NaN
    owed = [b * 8 + q for b in range(B) for q in range(6)] + [B * 8 + q for q in range(3)]
    ws, out, grad = h.out(n_ws, owed=owed), h.out(3), h.out(B, Tt)
    args = (d.data_ptr(), m2p.data_ptr(), tok.data_ptr(), _lib.ptr(sil), len(o['sil']) if sil is not None else 0, _lib.ptr(wdb), B, Tt, T,
            lam['lam_ph'], lam['lam_word'], lam['lam_sent'])
    h.call('dsf_dur_loss', *args, ws.data_ptr(), out.data_ptr())
    g = h.place(torch.tensor(gout, dtype=F32))
    h.call('dsf_dur_loss_bwd', *args, ws.data_ptr(), g.data_ptr(), grad.data_ptr())
    return dict(out=out, grad=grad, ws=ws)


def finish_dur(h, got, nan=False, no_word=False):
    if no_word:
        assert bool(torch.isfinite(got['out'][[0, 2]]).all()) and bool(torch.isfinite(got['grad']).all())
    h.finish(nan_ok=nan or no_word)


@pytest.mark.parametrize('c', V.dur_cases(), ids=V.dur_id)
def test_table_dur(h, c):
    """forward and backward of every duration row with a random grad_out"""
    f, o, gout = V.dur_flags(c), V.dur_operands(c), V.dur_gout(c)
    if f['no_word']:
        gout[1] = 0.0
    got = run_dur(h, o, gout, V.DUR_LAM)
    again = run_dur(h, o, gout, V.DUR_LAM)
    same_bits(got, again)
    finish_dur(h, got, f['nan'], f['no_word'])
    if f['nan']:                                                                # the header's `bad` path: NaN losses, NaN gradients
        assert bool(torch.isnan(got['out']).all()) and bool(torch.isnan(got['grad']).all())
        print(f'EDGE DUR | {V.dur_id(c)} | bad path: 3 NaN losses, {got["grad"].numel()} NaN gradients')
        return
    r64, r32 = V.dur_case_reference(c, F64), V.dur_case_reference(c, F32)
    res = {k: V.value_ratio(got['out'][i], r64['out'][i], r32['out'][i], V.FLOOR_DUR, 1e-3) for i, k in enumerate(('pdur', 'wdur', 'sdur'))
           if not (f['no_word'] and i == 1)}
    r, _, e, a = V.row_ratio(got['grad'], r64['grad'], r32['grad'], V.FLOOR_DUR)
    res['grad'] = (r, e, a)
    report('DUR', V.dur_id(c), res)


EXACT = (V.DurCase(3, 12, 3040, 'sil', 'long_phone'), V.DurCase(3, 12, 40, 'wdb', 'zero_frames'), V.DurCase(3, V.MAX_TXT, 3 * V.MAX_TXT, 'wdb', 'all_ones'),
         V.DurCase(3, 513, 1539, 'sil', 'pad_row'))


@pytest.mark.parametrize('c', EXACT, ids=V.dur_id)
def test_integer_durations_are_exact(h, c):
    """at dur_pred = log(dur_gt + 1) pdur is exactly 0: one frame counted wrong anywhere leaves log((g + 2) / (g + 1))^2 / phones > 0"""
    assert c in V.dur_cases()
    o = V.dur_operands(c)
    dur_gt = (LH.mel2ph_to_dur(o['mel2ph'], c.Tt) * (o['tok'] > 0)).float()
    o = dict(o, dur_pred=torch.log(dur_gt.to(DEV) + 1).cpu())
    got = run_dur(h, o, [1.0, 1.0, 1.0], V.DUR_LAM)
    finish_dur(h, got)
    assert float(got['out'][0]) == 0.0, float(got['out'][0])
    off = dict(o, mel2ph=o['mel2ph'].clone())
    off['mel2ph'][0, 0] = int(off['mel2ph'][0, 0]) % c.Tt + 1                   # one frame moved to another phone: no longer 0
    wrong = run_dur(h, off, [1.0, 1.0, 1.0], V.DUR_LAM)
    finish_dur(h, wrong)
    assert float(wrong['out'][0]) > 0.0


# ---- through losses.py ------------------------------------------------------------------------------------------------------------------
def test_losses_mel_loss_terms_on_the_strided_cwt_view(h):
    """the live cwt_loss: ssim path: output['cwt'][:, :, :10] of an 11-wide tensor, bias 20, no L1; the gradient flows into the parent, whose
    column 10 gets exactly zero"""
    c = V.MelCase(3, 33, 10, 20.0, 'tail', 'cwt')
    assert c in V.mel_cases()
    x, y = V.mel_operands(c)
    parent = torch.cat([x, torch.randn(c.B, c.T, 1, generator=V.gen(11))], 2).to(DEV).requires_grad_(True)
    view = parent[:, :, :10]
    assert view.stride() == (c.T * 11, 11, 1)
    out = losses.mel_loss_terms(view, y.to(DEV), bias=20.0, l1=False, ssim=True)
    out[1].backward()
    r64, r32 = (V.mel_reference(x, y, 20.0, 2, 1, (0.0, 1.0), (0.0, 1.0, 0.0), None, dt) for dt in (F64, F32))
    assert float(parent.grad[:, :, 10].abs().max()) == 0.0 and float(out[3]) == float(r64['out'][3]) and float(out[0]) == 0.0
    r, _, e, a = V.row_ratio(parent.grad[:, :, :10], r64['dx'], r32['dx'], V.FLOOR_MEL_GRAD)
    report('LOSSES', 'mel_loss_terms on cwt[:, :, :10], bias 20',
           dict(ssim=V.value_ratio(out[1], r64['out'][1], r32['out'][1], V.FLOOR_MEL_VALUE), S=V.value_ratio(out[2], r64['out'][2], r32['out'][2], V.FLOOR_MEL_VALUE),
                dx=(r, e, a)))


def test_losses_fs2_losses_with_cwt_loss_ssim():
    """fs2_losses on a synthetic output / sample with pitch_type cwt and cwt_loss: ssim against the restated objective
    (tests/test_gpu_fs2_loss.py's _objective_reference, its C term replaced by ssim_loss at bias 20)"""
    from tests.test_gpu_fs2_loss import LOSS_HP, SIL, _objective_reference
    B, T, Tt = 3, 33, 12
    hp = dict(LOSS_HP, cwt_loss='ssim', mel_loss='ssim:0.5|l1:0.5', use_pitch_embed=True, pitch_type='cwt', use_uv=True, use_energy_embed=False,
              lambda_ph_dur=0.7, lambda_word_dur=1.3, lambda_sent_dur=0.9, lambda_f0=0.8)
    mel_out, mels = V.mel_operands(V.MelCase(B, T, 80, 6.0, 'z16', 'contig'))
    cwt_x, cwt_y = V.mel_operands(V.MelCase(B, T, 10, 20.0, 'tail', 'cwt'))
    d = V.dur_operands(V.DurCase(B, Tt, T, 'sil', 'random'))
    g = V.gen(B, T, Tt, 99)
    leaves = dict(mel_out=mel_out, dur=d['dur_pred'], cwt=torch.cat([cwt_x, torch.randn(B, T, 1, generator=g)], 2), f0_mean=torch.rand(B, generator=g) + 6.5,
                  f0_std=torch.rand(B, generator=g) * 0.5 + 0.2)
    sample = dict(mels=mels, txt_tokens=d['tok'], mel2ph=d['mel2ph'], cwt_spec=cwt_y, uv=(torch.rand(B, T, generator=g) < 0.3).float(),
                  f0=torch.rand(B, T, generator=g), f0_mean=torch.rand(B, generator=g) + 6.5, f0_std=torch.rand(B, generator=g) * 0.5 + 0.2)

    def reference(dt):
        o = {k: v.to(dt).clone().requires_grad_(True) for k, v in leaves.items()}
        s = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sample.items()}
        L = _objective_reference(o, s, dict(hp, cwt_loss='l1'), 'fs2')                # its silence ids: SIL of that file
        L['C'] = LH.ssim_loss(o['cwt'][:, :, :10], s['cwt_spec'], 20.0) * hp['lambda_f0']
        sum(L.values()).backward()
        return {k: v.detach() for k, v in L.items()}, {k: v.grad for k, v in o.items()}

    (L64, g64), (L32, g32) = reference(F64), reference(F32)
    assert all(bool(torch.isfinite(v)) for v in L64.values()) and all(bool(torch.isfinite(v).all()) for v in g64.values())
    od = {k: v.to(DEV).requires_grad_(True) for k, v in leaves.items()}
    got = losses.fs2_losses(od, {k: v.to(DEV) for k, v in sample.items()}, hp, variant='fs2', sil_ph_ids=list(SIL))
    assert list(got) == list(L64), (list(got), list(L64))
    sum(got.values()).backward()
    floors = dict(mel_out=V.FLOOR_MEL_GRAD, cwt=V.FLOOR_MEL_GRAD, dur=V.FLOOR_DUR)
    res = {k: V.value_ratio(got[k], L64[k], L32[k], V.FLOOR_DUR if k.endswith('dur') else V.FLOOR_MEL_VALUE, 1e-3) for k in L64}
    for k, fl in floors.items():
        r, _, e, a = V.row_ratio(od[k].grad, g64[k], g32[k], fl)
        res['d' + k] = (r, e, a)
    report('LOSSES', 'fs2_losses, cwt_loss: ssim', res)


def test_losses_ssim_map_at_17_by_128():
    """ssim(..., size_average=False) at H = 17 (one frame past a tile), W = kMlMaxM, and the gradient of sum(map * R)"""
    c = V.MelCase(1, 17, V.MAX_M, 6.0, 'tail', 'contig')
    x, y = V.mel_operands(c)
    a, b, R = x[:, None] + 6.0, y[:, None] + 6.0, V.mel_grad_map(c) * x.numel()
    ad = a.to(DEV).requires_grad_(True)
    m = losses.ssim(ad, b.to(DEV), size_average=False)
    assert m.shape == (1, 17, V.MAX_M)
    (m * R.to(DEV)).sum().backward()
    ref = {}
    for dt in (F64, F32):
        ar = a.to(dt).requires_grad_(True)
        mr = LH.ssim_map(ar, b.to(dt)).mean(1)
        (mr * R.to(dt)).sum().backward()
        ref[dt] = (mr.detach(), ar.grad[:, 0])
    r1, _, e1, a1 = V.row_ratio(m, ref[F64][0], ref[F32][0], V.FLOOR_MEL_VALUE)
    r2, _, e2, a2 = V.row_ratio(ad.grad[:, 0], ref[F64][1], ref[F32][1], V.FLOOR_MEL_GRAD)
    report('LOSSES', 'ssim(size_average=False) H 17 W 128', dict(map=(r1, e1, a1), dx=(r2, e2, a2)))
