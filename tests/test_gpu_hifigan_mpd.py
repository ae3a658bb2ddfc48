"""GPU: the HiFi-GAN period discriminator (include/dsv.h section "HiFi-GAN period discriminator", csrc/hifigan_mpd.hpp) through the C ABI and
through diffsinger_amd.hifigan_disc, against the float64 restatement of tests/hifigan_mpd_helpers.py and the fixture recorded from the reference.

Per operator the comparison is the helpers' rule: |device - float64| <= bound element-wise, the bound built in float64 from the DEVICE'S OWN
operands (its saved activations and gradients, handed in as exact operands: every layer's bound starts afresh and no mask or sign can flip), never
from the code under test.  The layout is dense ([B][C][H][p], no padded tail), so "nothing beyond the valid samples" is shown on guards: every
buffer a kernel reads or writes lies between NaN-filled guard floats, which must stay NaN while every result stays finite and equal.

Shapes (p, T), for B in {1, 3} - the smallest at which each thing can go wrong:
    (2, 2)      heights 1, 1, 1, 1, 1: a window that is all padding but one sample; no reflect pad
    (11, 12)    2, 1, 1, 1, 1: the longest reflect pad (10), more rows than samples
    (3, 292)    98, 33, 11, 4, 2: an output tile of 32 + 1 rows; H0 = 2 mod 3
    (3, 300)    100, 34, 12, 4, 2: H0 = 1 mod 3, no pad
    (5, 1454)   291, 97, 33, 11, 4: H0 = 0 mod 3; the 33 seam one layer deeper
    (2, 2121)   1061, 354, 118, 40, 14: several workgroups along the positions, an odd T, the weight gradient's splits
    (2, 4100)   2050, 684, 228, 76, 26: the first layer's parameter gradient over 3 * 684 * 2 = 4104 positions at B = 3 - a second split of the edge
                kernel at K = 5, of 8 positions (one split at B = 1); the scale discriminator's T = 2121, B = 3 is the same seam at K = 15
    (7, 300), (11, 300)     43 .. 1 and 28 .. 1: the fixture's shape; positions no multiple of 32"""
import pytest
import torch

from tests import hifigan_mpd_helpers as MH
from tests.hifigan_disc_helpers import DEV, NAN, Guarded, Ops as _Ops, close, rnd, within

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (11, 12), (3, 292), (3, 300), (5, 1454), (2, 2121), (2, 4100), (7, 300), (11, 300)]
CASES = [(p, T, B) for p, T in SHAPES for B in (1, 3)]
CLOSE, CLOSE_LOSS = 1e-4, 1e-5          # the module-level figures of tests/test_hifigan_mpd_host.py


class Ops(_Ops):
    def pack(self, m):
        rows, ci, kt = m.shape
        m = m.contiguous()
        out = torch.empty(self.lib.dsv_packed_floats(rows, ci, kt), device=DEV)
        self.call('dsv_pack_weight', m.data_ptr(), rows, ci, kt, out.data_ptr())
        return out

    def pack_dgrad(self, w3, S):
        co, ci, _ = w3.shape
        out = torch.full((self.lib.dsv_hgp_dgrad_packed_offset(ci, co, S, S),), NAN, device=DEV)
        for r in range(S):
            m = self.lib.dsv_hgp_dgrad_phase_taps(S, r)
            ks = [k for k in range(5) if m >> k & 1]
            mat = w3[:, :, ks].permute(1, 0, 2).contiguous()
            self.call('dsv_pack_weight', mat.data_ptr(), ci, co, len(ks), out.data_ptr() + 4 * self.lib.dsv_hgp_dgrad_packed_offset(ci, co, S, r))
        return out


@pytest.fixture(scope='module')
def plain():
    """one seeded set of plain weights, shared and never modified: (float32 on the CPU, on the device as [Co][Ci][K], float64)"""
    ws, bs = MH.synth_plain(77)
    return ws, bs, [w[..., 0].contiguous().to(DEV) for w in ws], [b.to(DEV) for b in bs], [w.double() for w in ws], [b.double() for b in bs]


@pytest.mark.parametrize('p,T,B', CASES)
def test_operators_through_the_abi(plain, p, T, B):
    ws, bs, wd, bd, w64, b64 = plain
    o, gd = Ops(), Guarded()
    lib = o.lib
    hs = MH.heights(T, p)
    CH = [1] + [l[1] for l in MH.LAYERS]
    x = rnd(B, 1, T, seed=1000 * p + T)
    worst, worst1 = 0.0, 0.0                                    # sums under THE RULE; single roundings (their bound is attained)

    # ---- forward ----
    xw = gd.new(B, T + 3)                                       # rows 3 floats apart more than they are long: the gap stays NaN
    xw[:, :T] = x[:, 0].to(DEV)
    xf = gd.new(B, 1, hs[0], p)
    o.call('dsv_hgp_fold', xw.data_ptr(), xf.data_ptr(), B, T, T + 3, p)
    assert torch.equal(xf.cpu().double(), MH.fold64(x.double(), p)), 'fold'
    maps = [gd.new(B, CH[l + 1], hs[l + 1], p) for l in range(MH.N)]
    packed = [None] + [o.pack(wd[l]) for l in range(1, 5)]

    def forward(out):
        o.call('dsv_hgp_first', xf.data_ptr(), wd[0].data_ptr(), bd[0].data_ptr(), out[0].data_ptr(), B, 32, hs[0], p, 3, MH.SLOPE)
        for l in range(1, 5):
            ci, co, _, S = MH.LAYERS[l]
            o.call('dsv_hgp_conv', out[l - 1].data_ptr(), packed[l].data_ptr(), bd[l].data_ptr(), out[l].data_ptr(), B, ci, co, hs[l], p, S, MH.SLOPE)
        o.call('dsv_hgp_post', out[4].data_ptr(), wd[5].data_ptr(), bd[5].data_ptr(), out[5].data_ptr(), B, 1024, hs[5], p)
    forward(maps)
    m64 = [MH.d64(m) for m in maps]
    assert all(bool(torch.isfinite(m).all()) for m in m64)
    fw = MH.forward64(x.double(), p, w64, b64, inputs=m64)
    for l in range(MH.N):
        worst = max(worst, within(f'map {l}', maps[l], fw['fmap'][l], fw['e_fmap'][l]))
    again = [torch.empty_like(m) for m in maps]
    forward(again)
    assert all(torch.equal(a, m) for a, m in zip(again, maps)), 'two calls differ'

    # ---- backward: cotangents on the output and on every map ----
    g_out = rnd(B, hs[5] * p, seed=7)
    cots = [rnd(*m.shape, seed=10 + l, scale=0.5) for l, m in enumerate(maps)]
    g_out_d = gd.new(B, hs[5] * p, src=g_out)
    cots_d = [gd.new(*c.shape, src=c) for c in cots]
    ws_e = gd.new(max(lib.dsv_hgp_edge_workspace_floats(B, hs[5], p, 1024, 3), lib.dsv_hgp_edge_workspace_floats(B, hs[1], p, 32, 5)))
    dws = [gd.new(*w.shape[:3]) for w in ws]
    dbs = [gd.new(*b.shape) for b in bs]
    Gs = [gd.new(B, CH[l + 1], hs[l + 1], p) for l in range(5)]                 # gradient with respect to layer l's pre-activation

    def backward(dws, dbs, Gs, dxf, dx):
        o.call('dsv_hgp_post_backward', g_out_d.data_ptr(), cots_d[5].data_ptr(), maps[4].data_ptr(), wd[5].data_ptr(), cots_d[4].data_ptr(),
               ws_e.data_ptr(), dws[5].data_ptr(), dbs[5].data_ptr(), Gs[4].data_ptr(), B, 1024, hs[5], p, MH.SLOPE)
        for l in range(4, 0, -1):
            ci, co, _, S = MH.LAYERS[l]
            n = lib.dsv_hgp_wgrad_workspace_floats(B, ci, co, hs[l + 1], p)
            wsw = gd.new(n) if n else None
            o.call('dsv_hgp_conv_wgrad', Gs[l].data_ptr(), maps[l - 1].data_ptr(), o.p(wsw), dws[l].data_ptr(), dbs[l].data_ptr(), B, ci, co, hs[l], p, S)
            o.call('dsv_hgp_conv_dgrad', Gs[l].data_ptr(), o.pack_dgrad(wd[l], S).data_ptr(), cots_d[l - 1].data_ptr(), maps[l - 1].data_ptr(),
                   Gs[l - 1].data_ptr(), B, ci, co, hs[l], p, S, MH.SLOPE)
        o.call('dsv_hgp_first_backward', Gs[0].data_ptr(), xf.data_ptr(), wd[0].data_ptr(), ws_e.data_ptr(), dws[0].data_ptr(), dbs[0].data_ptr(),
               dxf.data_ptr(), B, 32, hs[0], p, 3)
        o.call('dsv_hgp_fold_backward', dxf.data_ptr(), dx.data_ptr(), B, T, p)
    dxf, dx = gd.new(B, 1, hs[0], p), gd.new(B, 1, T)
    backward(dws, dbs, Gs, dxf, dx)
    torch.cuda.synchronize()
    gd.check()
    for t in dws + dbs + Gs + [dxf, dx]:
        assert bool(torch.isfinite(t).all())
    # conv_post: the two cotangents are added in float32 (the same IEEE addition here), then exact operands
    G5 = (g_out.reshape(cots[5].shape) + cots[5]).double()
    G64 = [MH.d64(g) for g in Gs]
    for l in range(5, -1, -1):
        G = G5 if l == 5 else G64[l]
        a_in = m64[l - 1] if l > 0 else fw['xf']
        (dw, e_dw), (db, e_db) = MH.wgrad_bound(G, None, a_in, None, w64[l].shape, MH.geom(l))
        worst = max(worst, within(f'dw {l}', dws[l], dw[..., 0], e_dw[..., 0]), within(f'db {l}', dbs[l], db, e_db))
        D, e_D = MH.dgrad_bound(G, None, w64[l], a_in.shape[2], MH.geom(l))
        if l == 0:
            worst = max(worst, within('dxf', dxf, D, e_D))
            break
        D = D + cots[l - 1].double()
        e_D = e_D + MH.U * D.abs()
        m = MH.mask_of(m64[l - 1], MH.SLOPE)
        worst1 = max(worst1, within(f'G {l - 1}', Gs[l - 1], D * m, e_D * m + MH.U * (D * m).abs()))
    worst1 = max(worst1, within('dx', dx, *MH.fold_backward_bound(MH.d64(dxf), None, T, p)))
    dws2, dbs2, Gs2 = [torch.empty_like(t) for t in dws], [torch.empty_like(t) for t in dbs], [torch.empty_like(t) for t in Gs]
    dxf2, dx2 = torch.empty_like(dxf), torch.empty_like(dx)
    backward(dws2, dbs2, Gs2, dxf2, dx2)
    for a, b_ in zip(dws + dbs + Gs + [dxf, dx], dws2 + dbs2 + Gs2 + [dxf2, dx2]):
        assert torch.equal(a, b_), 'two calls differ'
    print(f'p={p} T={T} B={B}: worst error / bound {worst:.3f} (sums), {worst1:.3f} (single roundings)')


def test_optional_operands_and_refusals(plain):
    """no cotangent, no saved map, no bias, no second output cotangent; bad arguments return -1 with the message and launch nothing"""
    ws, bs, wd, bd, w64, b64 = plain
    o = Ops()
    lib, s = o.lib, o.s
    B, p, H = 2, 3, 7
    Ho = lib.dsv_hgp_height(H, 3)
    x = rnd(B, 32, H, p, seed=3)
    xd = x.to(DEV)
    out = torch.empty(B, 128, Ho, p, device=DEV)
    o.call('dsv_hgp_conv', xd.data_ptr(), o.pack(wd[1]).data_ptr(), None, out.data_ptr(), B, 32, 128, H, p, 3, MH.SLOPE)
    pre, e = MH.conv_bound(x.double(), w64[1], None, MH.geom(1))
    within('conv without bias', out, MH.leaky(pre, MH.SLOPE), e + MH.U * pre.abs())
    g = rnd(B, 128, Ho, p, seed=4)
    gdev = g.to(DEV)
    dxd = torch.empty(B, 32, H, p, device=DEV)
    o.call('dsv_hgp_conv_dgrad', gdev.data_ptr(), o.pack_dgrad(wd[1], 3).data_ptr(), None, None, dxd.data_ptr(), B, 32, 128, H, p, 3, MH.SLOPE)
    within('dgrad without cotangent and mask', dxd, *MH.dgrad_bound(g.double(), None, w64[1], H, MH.geom(1)))
    dw = torch.empty(128, 32, 5, device=DEV)
    o.call('dsv_hgp_conv_wgrad', gdev.data_ptr(), xd.data_ptr(), None, dw.data_ptr(), None, B, 32, 128, H, p, 3)
    (dw64, e_dw), _ = MH.wgrad_bound(g.double(), None, x.double(), None, w64[1].shape, MH.geom(1))
    within('wgrad without bias', dw, dw64[..., 0], e_dw[..., 0])
    a, b = xd.data_ptr(), out.data_ptr()
    err = lib.dsd_last_error
    assert lib.dsv_hgp_conv(a, a, None, b, B, 32, 100, H, p, 3, 0.1, s) == -1 and b'multiples of 32' in err()
    assert lib.dsv_hgp_conv(a, a, None, a + 4 * 40, B, 32, 128, H, p, 3, 0.1, s) == -1 and b'overlap' in err()
    assert lib.dsv_hgp_conv(a, a, None, b, B, 32, 128, 0, p, 3, 0.1, s) == -1 and b'bad shape' in err()
    assert lib.dsv_hgp_conv(a, a, None, b, 30000, 32, 128, H, p, 3, 0.1, s) == -1 and b'B * period <= 65535' in err()
    assert lib.dsv_hgp_fold(a, b, 1, 5, 5, 11, s) == -1 and b'reflect pad' in err()
    assert lib.dsv_hgp_conv_wgrad(a, a, None, b, None, 64, 32, 128, 100, p, 3, s) == -1 and b'need the workspace' in err()
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', [(1,), (3, 5, 7), (2, 32, 33, 3), (300001,)])
def test_feature_l1(shape):
    """float64 sums; sign(0) = 0; one element, odd sizes, more elements than one sweep of the grid (256 blocks x 256 threads x 4)"""
    from diffsinger_amd import hifigan_disc as HD
    r, g = rnd(*shape, seed=1), rnd(*shape, seed=2)
    g.reshape(-1)[::3] = r.reshape(-1)[::3]                     # ties: the gradient there is exactly zero
    r2, g2 = rnd(4, 9, seed=3), rnd(4, 9, seed=4)
    rd, gd_, r2d, g2d = (t.to(DEV).requires_grad_(True) for t in (r, g, r2, g2))
    n0 = HD.launch_count()
    loss = HD.feature_loss([[rd], [r2d]], [[gd_], [g2d]])
    assert HD.launch_count() - n0 == 3                          # n + 1
    want, e = MH.feature_loss64([[r.double()], [r2.double()]], [[g.double()], [g2.double()]])
    assert abs(float(loss) - float(want)) <= e + MH.U * abs(float(want)), (float(loss), float(want))
    (loss * 0.75).backward()
    assert HD.launch_count() - n0 == 5                          # + n
    for (a, b), (ga, gb) in (((r, g), (rd.grad, gd_.grad)), ((r2, g2), (r2d.grad, g2d.grad))):
        ct, e_ct = MH.l1_cotangents(a.double(), b.double())
        within('d/dr', ga, 0.75 * ct, 0.75 * e_ct + MH.U * ct.abs())
        assert torch.equal(gb, -ga)
    assert bool((rd.grad.reshape(-1)[::3] == 0).all())
    loss2 = HD.feature_loss([[rd.detach()], [r2d.detach()]], [[gd_.detach()], [g2d.detach()]])
    assert torch.equal(loss2, loss.detach())


def _op_inputs(plain, p, T, B, seed):
    ws, bs = plain[0], plain[1]
    x = rnd(B, 1, T, seed=seed)
    wl = [w.clone().to(DEV).requires_grad_(True) for w in ws]
    bl = [b.clone().to(DEV).requires_grad_(True) for b in bs]
    return x, wl, bl


@pytest.mark.parametrize('p,T,B', CASES)
def test_disc_p_op_end_to_end(plain, p, T, B):
    """forward and backward through ONE autograd node with cotangents on the output and on every map, against the restatement; the launch count"""
    from diffsinger_amd import _lib, hifigan_disc as HD
    lib = _lib.load()
    w64, b64 = plain[4], plain[5]
    x, wl, bl = _op_inputs(plain, p, T, B, 2000 * p + T)
    xd = x.to(DEV).requires_grad_(True)
    hs = MH.heights(T, p)
    n0 = HD.launch_count()
    out, fmap = HD.disc_p_op(xd, p, wl, bl)
    assert HD.launch_count() - n0 == 15
    assert out.shape == (B, hs[6] * p) and [tuple(m.shape) for m in fmap] == [(B, MH.LAYERS[l][1], hs[l + 1], p) for l in range(MH.N)]
    assert out.data_ptr() == fmap[5].data_ptr()                 # the output is the last map, flattened: a view
    fw = MH.forward64(x.double(), p, w64, b64)
    worst = 0.0
    for l in range(MH.N):
        worst = max(worst, within(f'map {l}', fmap[l], fw['fmap'][l], fw['e_fmap'][l]))
        err = float((MH.d64(fmap[l]) - fw['fmap'][l]).abs().max())
        assert err <= CLOSE * float(fw['fmap'][l].abs().max()), (l, err)
    g_out = rnd(*out.shape, seed=5)
    cots = [rnd(*m.shape, seed=20 + l, scale=0.5) for l, m in enumerate(fmap)]
    n1 = HD.launch_count()
    torch.autograd.backward([out] + fmap, [g_out.to(DEV)] + [c.to(DEV) for c in cots])
    s = sum(lib.dsv_hgp_wgrad_splits(B, MH.LAYERS[l][0], MH.LAYERS[l][1], hs[l + 1], p) > 1 for l in range(1, 5))
    assert HD.launch_count() - n1 == 37 + s + 2, (HD.launch_count() - n1, s)
    m64 = [MH.d64(m) for m in fmap]
    bw = MH.backward64(g_out.double(), [c.double() for c in cots], fw['xf'], T, p, w64, m64)
    worst = max(worst, within('dx', xd.grad, *bw['dx']))
    for l in range(MH.N):
        worst = max(worst, within(f'dw {l}', wl[l].grad, *bw['dw'][l]), within(f'db {l}', bl[l].grad, *bw['db'][l]))
        for got, (want, _) in ((wl[l].grad, bw['dw'][l]), (bl[l].grad, bw['db'][l])):
            assert float((MH.d64(got) - want).abs().max()) <= CLOSE * float(want.abs().max()), l
    assert float((MH.d64(xd.grad) - bw['dx'][0]).abs().max()) <= CLOSE * float(bw['dx'][0].abs().max())
    # no input gradient: two launches fewer
    out2, fmap2 = HD.disc_p_op(xd.detach(), p, wl, bl)
    n2 = HD.launch_count()
    out2.sum().backward()
    assert HD.launch_count() - n2 == 37 + s
    assert torch.equal(out2, out.detach())
    print(f'p={p} T={T} B={B}: worst error / chained bound {worst:.3g}')


@pytest.mark.parametrize('p,T', SHAPES)
def test_rows_are_batch_independent(plain, p, T):
    """op(cat(y, y_hat)) == cat(op(y), op(y_hat)) bit for bit, for halves of 1 and of 3 rows"""
    from diffsinger_amd import hifigan_disc as HD
    wl, bl = [w[..., None] for w in plain[2]], plain[3]
    for Bh in (1, 3):
        y, yh = rnd(Bh, 1, T, seed=31).to(DEV), rnd(Bh, 1, T, seed=32).to(DEV)
        with torch.no_grad():
            o2, f2 = HD.disc_p_op(torch.cat([y, yh]), p, wl, bl)
            (oa, fa), (ob, fb) = HD.disc_p_op(y, p, wl, bl), HD.disc_p_op(yh, p, wl, bl)
        assert torch.equal(o2, torch.cat([oa, ob]))
        for l in range(MH.N):
            assert torch.equal(f2[l], torch.cat([fa[l], fb[l]])), l


# ---- the modules at the fixture's shape ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fx():
    return MH.fixture()


@pytest.fixture(scope='module')
def inputs():
    return MH.fixture_inputs()


@pytest.fixture(scope='module')
def restated(inputs):
    state, y, y_hat = inputs
    return MH.mpd_forward64(state, y, y_hat)


def _module(state):
    from diffsinger_amd import MultiPeriodDiscriminator
    m = MultiPeriodDiscriminator()
    m.load_state_dict(state, strict=True)
    return m.to(DEV)


def test_modules_against_the_fixture_and_float64(fx, inputs, restated):
    from diffsinger_amd import hifigan_disc as HD
    state, y, y_hat = inputs
    m = _module(state)
    yh = y_hat.to(DEV).requires_grad_(True)
    n0 = HD.launch_count()
    rs, gs, frs, fgs = m(y.to(DEV), yh)
    fl = HD.feature_loss(frs, fgs)
    gen = HD.generator_loss(gs)
    rl, gl = HD.discriminator_loss(rs, gs)
    n1 = HD.launch_count()
    assert n1 - n0 == 5 * 15 + 31 + 10 + 20                     # five nodes, the feature loss over 30 pairs, 5 + 10 LSGAN means of two launches
    (fl + gen + rl + gl).backward()
    hs = [MH.heights(MH.FIXTURE_T, p) for p in MH.PERIODS]
    s = sum(HD._lib.load().dsv_hgp_wgrad_splits(2, MH.LAYERS[l][0], MH.LAYERS[l][1], h[l + 1], p) > 1 for h, p in zip(hs, MH.PERIODS) for l in range(1, 5))
    assert HD.launch_count() - n1 == 5 * (37 + 2) + s + 30 + 15  # no launch beyond the operators': no feature map or cotangent is copied by the library
    # the fixture: the reference's own float32 numbers
    for i in range(5):
        close(f'r{i}', rs[i], torch.from_numpy(fx[f'r{i}']).double())
        close(f'g{i}', gs[i], torch.from_numpy(fx[f'g{i}']).double())
        for l in range(MH.N):
            for sname, maps in (('r', frs), ('g', fgs)):
                full = MH.d64(maps[i][l]).reshape(-1)
                assert tuple(maps[i][l].shape) == tuple(restated[sname][i]['fmap'][l].shape)
                close(f'f{sname}{i}_{l}', full[torch.from_numpy(fx[f'idx/f{sname}{i}_{l}']).long()], torch.from_numpy(fx[f'f{sname}{i}_{l}']).double(), full)
    for name, got, want in zip(('feature', 'generator', 'r', 'g'), (fl, gen, rl, gl), fx['losses']):
        rel = abs(float(got) - float(want)) / abs(float(want))
        print(f'{name}_loss: relative error {rel:.3e}')
        assert rel <= CLOSE_LOSS, (name, float(got), float(want))
    close('dy_hat', yh.grad, torch.from_numpy(fx['dy_hat']).double())
    grads = dict(m.named_parameters())
    assert len(grads) == 90
    for k, prm in grads.items():
        full = MH.d64(prm.grad).reshape(-1)
        close('grad/' + k, full[torch.from_numpy(fx['idx/grad/' + k]).long()], torch.from_numpy(fx['grad/' + k]).double(), full)
    # float64: the device's error on every forward tensor is at most 4 x the fp32 CPU twin's own, floor 2e-6 of the tensor's largest value
    twin = MH.TwinMPD()
    twin.load_state_dict(state, strict=True)
    with torch.no_grad():
        trs, tgs, tfrs, tfgs = twin(y, y_hat)
    for i in range(5):
        for l in range(MH.N):
            for sname, maps, tmaps in (('r', frs, tfrs), ('g', fgs, tfgs)):
                want = restated[sname][i]['fmap'][l]
                big = float(want.abs().max())
                e_dev = float((MH.d64(maps[i][l]) - want).abs().max()) / big
                e_cpu = float((tmaps[i][l].double() - want).abs().max()) / big
                assert e_dev <= max(4 * e_cpu, 2e-6), (sname, i, l, e_dev, e_cpu)
    # remove_weight_norm() leaves the outputs bit-equal
    m.remove_weight_norm()
    with torch.no_grad():
        rs2, gs2, frs2, fgs2 = m(y.to(DEV), y_hat.to(DEV))
    for i in range(5):
        assert torch.equal(rs2[i], rs[i]) and torch.equal(gs2[i], gs[i])
        for l in range(MH.N):
            assert torch.equal(frs2[i][l], frs[i][l]) and torch.equal(fgs2[i][l], fgs[i][l])


def test_one_batch_of_two_equals_two_calls(inputs):
    """the module runs d(y) and d(y_hat) as one batch; the reference makes two calls: same bits"""
    state, y, y_hat = inputs
    m = _module(state)
    with torch.no_grad():
        rs, gs, frs, fgs = m(y.to(DEV), y_hat.to(DEV))
        for i, d in enumerate(m.discriminators):
            r, fr = d(y.to(DEV))
            g, fg = d(y_hat.to(DEV))
            assert torch.equal(r, rs[i]) and torch.equal(g, gs[i])
            for l in range(MH.N):
                assert torch.equal(fr[l], frs[i][l]) and torch.equal(fg[l], fgs[i][l])


def test_generator_and_discriminator_side_losses(inputs, restated):
    """one backward of each objective from a fixed y_hat leaf (the generator is not run), against the float64 restatement"""
    from diffsinger_amd import hifigan_adversarial_losses, hifigan_discriminator_losses
    state, y, y_hat = inputs
    fl64, gen64, rl64, gl64 = MH.mpd_losses64(restated)

    def rel(name, got, want):
        r = abs(float(got) - float(want)) / abs(float(want))
        print(f'{name}: relative error {r:.3e}')
        assert r <= CLOSE_LOSS, (name, float(got), float(want))
    # the generator's side
    m = _module(state)
    yh = y_hat.to(DEV).requires_grad_(True)
    losses = hifigan_adversarial_losses(m, y.to(DEV), yh)
    assert sorted(losses) == ['adv', 'fm']
    rel('adv', losses['adv'], gen64)
    rel('fm', losses['fm'], fl64)
    (losses['adv'] + losses['fm']).backward()
    bw = MH.mpd_backward64(restated, state, MH.FIXTURE_T, 1.0, 1.0, 0.0, 0.0)
    assert yh.grad is not None
    close('generator side dy_hat', yh.grad, bw['dy_hat'][0])
    for k, prm in m.named_parameters():
        close('generator side grad/' + k, prm.grad, bw['grads'][k][0])
    # the discriminator's side: y_hat is detached
    m = _module(state)
    yh = y_hat.to(DEV).requires_grad_(True)
    rl, gl = hifigan_discriminator_losses(m, y.to(DEV), yh)
    rel('r_loss', rl, rl64)
    rel('g_loss', gl, gl64)
    (rl + gl).backward()
    assert yh.grad is None
    bw = MH.mpd_backward64(restated, state, MH.FIXTURE_T, 0.0, 0.0, 1.0, 1.0)
    for k, prm in m.named_parameters():
        close('discriminator side grad/' + k, prm.grad, bw['grads'][k][0])
