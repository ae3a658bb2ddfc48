"""GPU: the HiFi-GAN scale discriminator's stack (include/dsv.h section "HiFi-GAN scale discriminator stack", csrc/hifigan_msd.hpp) through the C ABI
and through diffsinger_amd.hifigan_disc, against the float64 restatement of tests/hifigan_disc_helpers.py and the fixture recorded from the reference.

Per operator the comparison is the helpers' rule: |device - float64| <= bound element-wise, the bound built in float64 from the DEVICE'S OWN operands
(its saved activations and gradients, handed in as exact operands: every layer's bound starts afresh and no mask can flip), never from the code under
test.  The layout is dense ([B][C][L], no padded tail), so "nothing beyond the valid samples" is shown on guards: every buffer a kernel reads or
writes lies between NaN-filled guard floats, which must stay NaN while every result stays finite and equal on a second call.

Shapes T, for B in {1, 3} - the smallest at which each thing can go wrong (per-layer lengths: tests/test_hifigan_msd_host.py):
    1       1, 1, 1, 1, 1: every window is padding but one sample
    41      41, 21, 11, 3, 1: rows shorter than the kernel at every grouped layer
    280     .. 70, 18, 5 and 300 .. 75, 19, 5: the inputs of the stride-4 layers are 2 and 3 mod 4; 300 is the fixture's shape
    513     513, 257, 129, 33, 9: one past a power of two at every layer - a one-position remainder tile whatever the tile size
    1024    all lengths multiples of the strides and of the tiles
    1030    1030, 515, 258, 65, 17: even / odd / 2 mod 4 / 1 mod 4
    2121    2121, 1061, 531, 133, 34: odd, several workgroups along the positions, the weight gradient's splits engaged (B 3)"""
import copy

import pytest
import torch

from tests import hifigan_disc_helpers as DH
from tests import hifigan_msd_helpers as SH
from tests.hifigan_disc_helpers import DEV, Guarded, Ops as _Ops, close, rnd, within

pytestmark = pytest.mark.gpu

TS = [1, 41, 280, 300, 513, 1024, 1030, 2121]
CASES = [(T, B) for T in TS for B in (1, 3)]
CLOSE, CLOSE_LOSS, CLOSE_UNIT = 1e-4, 1e-5, 1e-5        # the module-level figures of tests/test_hifigan_disc_host.py
N = DH.N


class Ops(_Ops):
    def pack_dense(self, m):
        rows, ci, kt = m.shape
        m = m.contiguous()
        out = torch.empty(self.lib.dsv_packed_floats(rows, ci, kt), device=DEV)
        self.call('dsv_pack_weight', m.data_ptr(), rows, ci, kt, out.data_ptr())
        return out

    def pack(self, w, l, dgrad, gd=None):
        ci, co, _, s, g = DH.LAYERS[l]
        n = self.lib.dsv_hgs_packed_floats(ci, co, s, g, dgrad)
        out = gd.new(n) if gd is not None else torch.empty(n, device=DEV)
        self.call('dsv_hgs_pack', w.data_ptr(), out.data_ptr(), ci, co, s, g, dgrad)
        return out


@pytest.fixture(scope='module')
def plain():
    """one seeded set of plain weights, shared and never modified: (float32 on the CPU, on the device, float64)"""
    ws, bs = DH.synth_plain(77)
    return ws, bs, [w.contiguous().to(DEV) for w in ws], [b.to(DEV) for b in bs], [w.double() for w in ws], [b.double() for b in bs]


def _abi_case(plain, T, B):
    ws, bs, wd, bd, w64, b64 = plain
    o, gd = Ops(), Guarded()
    lib = o.lib
    ls = DH.lengths(T)
    CO = [l[1] for l in DH.LAYERS]
    x = rnd(B, 1, T, seed=1000 + T)
    worst, worst1 = 0.0, 0.0                                    # sums under THE RULE; single roundings

    # ---- forward ----
    ld = T + 3                                                  # rows 3 floats apart more than they are long: the gap stays NaN
    xw = gd.new(B, ld)
    xw[:, :T] = x[:, 0].to(DEV)
    maps = [gd.new(B, CO[l], ls[l]) for l in range(N)]
    packed = [None] + [o.pack(wd[l], l, 0, gd) for l in range(1, 6)] + [o.pack_dense(wd[6])]

    def forward(out):
        o.call('dsv_hgs_first', xw.data_ptr(), wd[0].data_ptr(), bd[0].data_ptr(), out[0].data_ptr(), B, 128, T, ld, DH.SLOPE)
        for l in range(1, 6):
            ci, co, _, s, g = DH.LAYERS[l]
            o.call('dsv_hgs_gconv', out[l - 1].data_ptr(), packed[l].data_ptr(), bd[l].data_ptr(), out[l].data_ptr(), B, ci, co, ls[l - 1], s, g, DH.SLOPE)
        o.call('dsv_hgp_conv', out[5].data_ptr(), packed[6].data_ptr(), bd[6].data_ptr(), out[6].data_ptr(), B, 1024, 1024, ls[5], 1, 1, DH.SLOPE)
        o.call('dsv_hgp_post', out[6].data_ptr(), wd[7].data_ptr(), bd[7].data_ptr(), out[7].data_ptr(), B, 1024, ls[7], 1)
    forward(maps)
    m64 = [DH.d64(m) for m in maps]
    assert all(bool(torch.isfinite(m).all()) for m in m64)
    fw = DH.forward64(x.double(), w64, b64, inputs=m64)
    for l in range(N):
        worst = max(worst, within(f'map {l}', maps[l], fw['fmap'][l], fw['e_fmap'][l]))
    again = [torch.empty_like(m) for m in maps]
    forward(again)
    assert all(torch.equal(a, m) for a, m in zip(again, maps)), 'two calls differ'

    # ---- backward: cotangents on the output and on every map ----
    g_out = rnd(B, ls[7], seed=7)
    cots = [rnd(*m.shape, seed=10 + l, scale=0.5) for l, m in enumerate(maps)]
    g_out_d = gd.new(B, ls[7], src=g_out)
    cots_d = [gd.new(*c.shape, src=c) for c in cots]
    ws_e = gd.new(lib.dsv_hgp_edge_workspace_floats(B, ls[7], 1, 1024, 3))
    ws_f = gd.new(lib.dsv_hgs_first_workspace_floats(B, T, 128))
    dws = [gd.new(*w.shape) for w in ws]
    dbs = [gd.new(*b.shape) for b in bs]
    Gs = [gd.new(B, CO[l], ls[l]) for l in range(7)]           # gradient with respect to layer l's pre-activation
    packed_b = [None] + [o.pack(wd[l], l, 1, gd) for l in range(1, 6)] + [o.pack_dense(wd[6].permute(1, 0, 2))]
    wsw = [None] * 7
    for l in range(1, 6):
        ci, co, _, s, g = DH.LAYERS[l]
        n = lib.dsv_hgs_wgrad_workspace_floats(B, ci, co, ls[l], s, g)
        wsw[l] = gd.new(n) if n else None
    n = lib.dsv_hgp_wgrad_workspace_floats(B, 1024, 1024, ls[6], 1)
    wsw[6] = gd.new(n) if n else None

    def backward(dws, dbs, Gs, dx):
        o.call('dsv_hgp_post_backward', g_out_d.data_ptr(), cots_d[7].data_ptr(), maps[6].data_ptr(), wd[7].data_ptr(), cots_d[6].data_ptr(),
               ws_e.data_ptr(), dws[7].data_ptr(), dbs[7].data_ptr(), Gs[6].data_ptr(), B, 1024, ls[7], 1, DH.SLOPE)
        o.call('dsv_hgp_conv_wgrad', Gs[6].data_ptr(), maps[5].data_ptr(), o.p(wsw[6]), dws[6].data_ptr(), dbs[6].data_ptr(), B, 1024, 1024, ls[5], 1, 1)
        o.call('dsv_hgp_conv_dgrad', Gs[6].data_ptr(), packed_b[6].data_ptr(), cots_d[5].data_ptr(), maps[5].data_ptr(), Gs[5].data_ptr(), B, 1024, 1024,
               ls[5], 1, 1, DH.SLOPE)
        for l in range(5, 0, -1):
            ci, co, _, s, g = DH.LAYERS[l]
            o.call('dsv_hgs_gconv_wgrad', Gs[l].data_ptr(), maps[l - 1].data_ptr(), o.p(wsw[l]), dws[l].data_ptr(), dbs[l].data_ptr(), B, ci, co, ls[l - 1],
                   s, g)
            o.call('dsv_hgs_gconv_dgrad', Gs[l].data_ptr(), packed_b[l].data_ptr(), cots_d[l - 1].data_ptr(), maps[l - 1].data_ptr(), Gs[l - 1].data_ptr(),
                   B, ci, co, ls[l - 1], s, g, DH.SLOPE)
        o.call('dsv_hgs_first_backward', Gs[0].data_ptr(), xw.data_ptr(), wd[0].data_ptr(), ws_f.data_ptr(), dws[0].data_ptr(), dbs[0].data_ptr(),
               dx.data_ptr(), B, 128, T, ld)
    dx = gd.new(B, 1, T)
    backward(dws, dbs, Gs, dx)
    torch.cuda.synchronize()
    gd.check()
    for t in dws + dbs + Gs + [dx]:
        assert bool(torch.isfinite(t).all())
    # conv_post: the two cotangents are added in float32 (the same IEEE addition here), then exact operands
    G7 = (g_out.reshape(cots[7].shape) + cots[7]).double()
    G64 = [DH.d64(g) for g in Gs]
    for l in range(N - 1, -1, -1):
        G = G7 if l == N - 1 else G64[l]
        a_in = m64[l - 1] if l > 0 else x.double()
        (dw, e_dw), (db, e_db) = DH.wgrad_bound(G, None, a_in, None, w64[l].shape, DH.geom(l))
        worst = max(worst, within(f'dw {l}', dws[l], dw, e_dw), within(f'db {l}', dbs[l], db, e_db))
        D, e_D = DH.dgrad_bound(G, None, w64[l], a_in.shape[2], DH.geom(l))
        if l == 0:
            worst = max(worst, within('dx', dx, D, e_D))
            break
        D = D + cots[l - 1].double()
        e_D = e_D + DH.U * D.abs()
        m = DH.mask_of(m64[l - 1], DH.SLOPE)
        worst1 = max(worst1, within(f'G {l - 1}', Gs[l - 1], D * m, e_D * m + DH.U * (D * m).abs()))
    dws2, dbs2, Gs2, dx2 = [torch.empty_like(t) for t in dws], [torch.empty_like(t) for t in dbs], [torch.empty_like(t) for t in Gs], torch.empty_like(dx)
    backward(dws2, dbs2, Gs2, dx2)
    for a, b_ in zip(dws + dbs + Gs + [dx], dws2 + dbs2 + Gs2 + [dx2]):
        assert torch.equal(a, b_), 'two calls differ'
    torch.cuda.synchronize()
    gd.check()
    print(f'T={T} B={B}: worst error / bound {worst:.3f} (sums), {worst1:.3f} (single roundings)')


@pytest.mark.parametrize('T,B', CASES)
def test_operators_through_the_abi(plain, T, B):
    _abi_case(plain, T, B)


def test_optional_operands_and_refusals(plain):
    """no bias, no cotangent, no saved map, no dx, no db; a cotangent on only some maps; nothing arriving on out; a bad geometry launches nothing"""
    from diffsinger_amd import hifigan_disc as HD
    ws, bs, wd, bd, w64, b64 = plain
    o = Ops()
    lib, s = o.lib, o.s
    B, L, l = 2, 37, 3                                          # 256 -> 512, stride 4, 16 groups
    ci, co, _, S, g = DH.LAYERS[l]
    Lo = lib.dsv_hgs_out_len(L, S)
    x = rnd(B, ci, L, seed=3)
    xd = x.to(DEV)
    out = torch.empty(B, co, Lo, device=DEV)
    o.call('dsv_hgs_gconv', xd.data_ptr(), o.pack(wd[l], l, 0).data_ptr(), None, out.data_ptr(), B, ci, co, L, S, g, DH.SLOPE)
    pre, e = DH.conv_bound(x.double(), w64[l], None, DH.geom(l))
    within('gconv without bias', out, DH.leaky(pre, DH.SLOPE), e + DH.U * pre.abs())
    gr = rnd(B, co, Lo, seed=4)
    grd = gr.to(DEV)
    dxd = torch.empty(B, ci, L, device=DEV)
    o.call('dsv_hgs_gconv_dgrad', grd.data_ptr(), o.pack(wd[l], l, 1).data_ptr(), None, None, dxd.data_ptr(), B, ci, co, L, S, g, DH.SLOPE)
    within('dgrad without cotangent and mask', dxd, *DH.dgrad_bound(gr.double(), None, w64[l], L, DH.geom(l)))
    dw = torch.empty(co, ci // g, 41, device=DEV)
    o.call('dsv_hgs_gconv_wgrad', grd.data_ptr(), xd.data_ptr(), None, dw.data_ptr(), None, B, ci, co, L, S, g)
    (dw64, e_dw), _ = DH.wgrad_bound(gr.double(), None, x.double(), None, w64[l].shape, DH.geom(l))
    within('wgrad without bias', dw, dw64, e_dw)
    # first layer: no bias; backward without db and dx
    T = 50
    x0 = rnd(B, 1, T, seed=5)
    x0d = x0.to(DEV)
    a0 = torch.empty(B, 128, T, device=DEV)
    o.call('dsv_hgs_first', x0d.data_ptr(), wd[0].data_ptr(), None, a0.data_ptr(), B, 128, T, T, DH.SLOPE)
    pre, e = DH.conv_bound(x0.double(), w64[0], None, DH.geom(0))
    within('first without bias', a0, DH.leaky(pre, DH.SLOPE), e + DH.U * pre.abs())
    g0 = rnd(B, 128, T, seed=6)
    g0d = g0.to(DEV)
    dw0 = torch.empty(128, 1, 15, device=DEV)
    wsf = torch.empty(lib.dsv_hgs_first_workspace_floats(B, T, 128), device=DEV)
    o.call('dsv_hgs_first_backward', g0d.data_ptr(), x0d.data_ptr(), wd[0].data_ptr(), wsf.data_ptr(), dw0.data_ptr(), None, None, B, 128, T, T)
    (dw64, e_dw), _ = DH.wgrad_bound(g0.double(), None, x0.double(), None, w64[0].shape, DH.geom(0))
    within('first wgrad without db and dx', dw0, dw64, e_dw)
    a, b = xd.data_ptr(), out.data_ptr()
    err = lib.dsd_last_error
    n0 = HD.launch_count()
    assert lib.dsv_hgs_gconv(a, a, None, b, B, 256, 512, L, 2, 16, 0.1, s) == -1 and b'none of the grouped layers' in err()
    assert lib.dsv_hgs_gconv(a, a, None, a + 4 * 40, B, ci, co, L, S, g, 0.1, s) == -1 and b'overlap' in err()
    assert lib.dsv_hgs_gconv_dgrad(a, a, None, None, b, B, ci, co, 0, S, g, 0.1, s) == -1 and b'bad shape' in err()
    assert lib.dsv_hgs_gconv_wgrad(a, a, None, b, None, 3, 128, 128, 2121, 2, 4, s) == -1 and b'need the workspace' in err()
    # the node: no bias on two layers, a cotangent on only some maps, nothing arriving on out
    T = 300
    xx = rnd(B, 1, T, seed=8)
    wl = [w.clone().requires_grad_(True) for w in wd]
    bl = [None if i in (2, 6) else t.clone().requires_grad_(True) for i, t in enumerate(bd)]
    xg = xx.to(DEV).requires_grad_(True)
    out, fmap = HD.disc_s_op(xg, wl, bl)
    b64n = [None if i in (2, 6) else t for i, t in enumerate(b64)]
    fw = DH.forward64(xx.double(), w64, b64n)
    for i in range(N):
        close(f'map {i} (no bias on 2, 6)', fmap[i], fw['fmap'][i])
    cots = [None] * N
    cots[1], cots[4] = rnd(*fmap[1].shape, seed=11), rnd(*fmap[4].shape, seed=12)
    n1 = HD.launch_count()
    torch.autograd.backward([fmap[1], fmap[4]], [cots[1].to(DEV), cots[4].to(DEV)])
    sp = sum(lib.dsv_hgs_wgrad_splits(B, DH.LAYERS[i][0], DH.LAYERS[i][1], DH.lengths(T)[i], DH.LAYERS[i][3], DH.LAYERS[i][4]) > 1 for i in range(1, 6))
    assert HD.launch_count() - n1 == 30 + sp + 1 - 2            # two layers without a bias gradient
    bw = DH.backward64(None, [None if c is None else c.double() for c in cots], xx.double(), w64, [DH.d64(m) for m in fmap])
    close('dx', xg.grad, bw['dx'][0])
    for i in range(N):
        if i <= 4:
            close(f'dw {i}', wl[i].grad, bw['dw'][i][0])
        else:                                                   # above the topmost cotangent nothing arrives: exact zeros
            assert not bool(wl[i].grad.any()) and (bl[i] is None or not bool(bl[i].grad.any()))
    assert bl[2] is None and bl[3].grad is not None
    torch.cuda.synchronize()


@pytest.mark.parametrize('T,B', CASES)
def test_disc_s_op_end_to_end(plain, T, B):
    """forward and backward through ONE autograd node with cotangents on the output and on every map, against the restatement; the launch count.
    The forward reference is built from the input alone.  The backward reference takes its leaky-ReLU masks and its weight-gradient operands from
    the DEVICE'S maps, by design: at random data some activation always lies within its float32 bound of zero, where the float64 mask may be the
    other one and the two gradients are different functions.  Those maps are held to float64 just above; a backward from the input alone is
    compared at the fixture's shape, where no mask is in doubt (test_modules_against_the_fixture_and_float64)."""
    from diffsinger_amd import _lib, hifigan_disc as HD
    lib = _lib.load()
    ws, bs, wd, bd, w64, b64 = plain
    x = rnd(B, 1, T, seed=2000 + T)
    wl = [w.clone().requires_grad_(True) for w in wd]
    bl = [b.clone().requires_grad_(True) for b in bd]
    xd = x.to(DEV).requires_grad_(True)
    ls = DH.lengths(T)
    n0 = HD.launch_count()
    out, fmap = HD.disc_s_op(xd, wl, bl)
    assert HD.launch_count() - n0 == 15
    assert out.shape == (B, ls[7]) and [tuple(m.shape) for m in fmap] == [(B, DH.LAYERS[l][1], ls[l]) for l in range(N)]
    assert out.data_ptr() == fmap[7].data_ptr()                 # the output is the last map, flattened: a view
    fw = DH.forward64(x.double(), w64, b64)
    worst = 0.0
    for l in range(N):
        worst = max(worst, within(f'map {l}', fmap[l], fw['fmap'][l], fw['e_fmap'][l]))
        close(f'map {l}', fmap[l], fw['fmap'][l])
    g_out = rnd(*out.shape, seed=5)
    cots = [rnd(*m.shape, seed=20 + l, scale=0.5) for l, m in enumerate(fmap)]
    n1 = HD.launch_count()
    torch.autograd.backward([out] + fmap, [g_out.to(DEV)] + [c.to(DEV) for c in cots])
    sp = sum(lib.dsv_hgs_wgrad_splits(B, DH.LAYERS[l][0], DH.LAYERS[l][1], ls[l], DH.LAYERS[l][3], DH.LAYERS[l][4]) > 1 for l in range(1, 6))
    sp += lib.dsv_hgp_wgrad_splits(B, 1024, 1024, ls[6], 1) > 1
    # conv_post 3, the dense layer 5, per grouped layer 4 (+ 1 where the weight gradient splits), the first layer 2 + 1 for dx
    assert HD.launch_count() - n1 == 30 + sp + 1, (HD.launch_count() - n1, sp)
    m64 = [DH.d64(m) for m in fmap]
    bw = DH.backward64(g_out.double(), [c.double() for c in cots], x.double(), w64, m64)
    worst = max(worst, within('dx', xd.grad, *bw['dx']))
    close('dx', xd.grad, bw['dx'][0])
    for l in range(N):
        worst = max(worst, within(f'dw {l}', wl[l].grad, *bw['dw'][l]), within(f'db {l}', bl[l].grad, *bw['db'][l]))
        close(f'dw {l}', wl[l].grad, bw['dw'][l][0])
        close(f'db {l}', bl[l].grad, bw['db'][l][0])
    # no input gradient: one launch fewer
    out2, fmap2 = HD.disc_s_op(xd.detach(), wl, bl)
    n2 = HD.launch_count()
    out2.sum().backward()
    assert HD.launch_count() - n2 == 30 + sp
    assert torch.equal(out2, out.detach())
    print(f'T={T} B={B}: worst error / chained bound {worst:.3g}')


@pytest.mark.parametrize('T', TS)
def test_rows_are_batch_independent(plain, T):
    """op(cat(y, y_hat)) == cat(op(y), op(y_hat)) bit for bit, forward and data gradient, for halves of 1 and of 3 rows"""
    from diffsinger_amd import hifigan_disc as HD
    wl, bl = plain[2], plain[3]
    for Bh in (1, 3):
        y, yh = rnd(Bh, 1, T, seed=31).to(DEV), rnd(Bh, 1, T, seed=32).to(DEV)
        yy = torch.cat([y, yh]).requires_grad_(True)
        ya, yb = y.clone().requires_grad_(True), yh.clone().requires_grad_(True)
        o2, f2 = HD.disc_s_op(yy, wl, bl)
        (oa, fa), (ob, fb) = HD.disc_s_op(ya, wl, bl), HD.disc_s_op(yb, wl, bl)
        assert torch.equal(o2, torch.cat([oa, ob]))
        for l in range(N):
            assert torch.equal(f2[l], torch.cat([fa[l], fb[l]])), l
        cots = [rnd(*m.shape, seed=40 + l).to(DEV) for l, m in enumerate(f2)]
        torch.autograd.backward(f2, cots)
        torch.autograd.backward(fa, [c[:Bh] for c in cots])
        torch.autograd.backward(fb, [c[Bh:] for c in cots])
        assert torch.equal(yy.grad, torch.cat([ya.grad, yb.grad]))


# ---- the modules at the fixture's shape ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fx():
    return DH.fixture()


@pytest.fixture(scope='module')
def inputs():
    """the fixture's recipe with discriminator 0's spectral buffers from their recording: the same state on every host (tests/hifigan_msd_helpers.py)"""
    return SH.fixture_inputs()


@pytest.fixture(scope='module')
def restated(inputs):
    """the float64 restatement in both modes, computed once: {mode: (forward, backward)}"""
    state, y, y_hat = inputs
    out = {}
    for mode in ('eval', 'train'):
        fw = DH.msd_forward64(state, y, y_hat, mode == 'train')
        out[mode] = (fw, DH.msd_backward64(fw, state, DH.FIXTURE_T))
    return out


def _module(state, training):
    from diffsinger_amd import MultiScaleDiscriminator
    m = MultiScaleDiscriminator()
    m.load_state_dict(state, strict=True)
    return m.to(DEV).train(training)


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_modules_against_the_fixture_and_float64(fx, inputs, restated, mode):
    from diffsinger_amd import hifigan_disc as HD
    state, y, y_hat = inputs
    fw, bw = restated[mode]
    m = _module(state, mode == 'train')
    yh = y_hat.to(DEV).requires_grad_(True)
    n0 = HD.launch_count()
    rs, gs, frs, fgs = m(y.to(DEV), yh)
    nodes = 4 if mode == 'train' else 3
    assert HD.launch_count() - n0 == nodes * 15 + 2             # the nodes and the two poolings of the pair
    fl = HD.feature_loss(frs, fgs)
    gen = HD.generator_loss(gs)
    rl, gl = HD.discriminator_loss(rs, gs)
    (fl + gen + rl + gl).backward()
    for i in range(3):
        for sname, outs, maps in (('r', rs, frs), ('g', gs, fgs)):
            f = fw[sname][i]
            want = torch.from_numpy(fx[f'{mode}/{sname}{i}']).double()
            close(f'{mode} {sname}{i}', outs[i], want)
            within(f'{mode} {sname}{i} float64', outs[i], f['fmap'][N - 1].reshape(want.shape), f['e_fmap'][N - 1].reshape(want.shape))
            for l in range(N):
                assert tuple(maps[i][l].shape) == tuple(f['fmap'][l].shape)
                full = DH.d64(maps[i][l]).reshape(-1)
                idx = torch.from_numpy(fx[f'idx/f{sname}{i}_{l}']).long()
                close(f'{mode} f{sname}{i}_{l}', full[idx], torch.from_numpy(fx[f'{mode}/f{sname}{i}_{l}']).double(), full)
                within(f'{mode} f{sname}{i}_{l} float64', maps[i][l], f['fmap'][l], f['e_fmap'][l])
                close(f'{mode} f{sname}{i}_{l} float64', maps[i][l], f['fmap'][l])
    for name, got, want, want64, e in zip(('feature', 'generator', 'r', 'g'), (t.detach() for t in (fl, gen, rl, gl)), fx[f'{mode}/losses'], DH.msd_losses64(fw), DH.msd_loss_bounds(fw)):
        rel = abs(float(got) - float(want)) / abs(float(want))
        print(f'{mode} {name}_loss: relative error {rel:.3e}')
        assert rel <= CLOSE_LOSS, (name, float(got), float(want))
        assert abs(float(got) - float(want64)) <= e + 64 * DH.U * abs(float(want64)), name
        assert abs(float(got) - float(want64)) <= CLOSE_LOSS * abs(float(want64)), name
    close(f'{mode} dy_hat', yh.grad, torch.from_numpy(fx[f'{mode}/dy_hat']).double())
    within(f'{mode} dy_hat float64', yh.grad, *bw['dy_hat'])
    close(f'{mode} dy_hat float64', yh.grad, bw['dy_hat'][0])
    grads = dict(m.named_parameters())
    assert len(grads) == 64 and sorted(grads) == sorted(bw['grads'])
    for k, prm in grads.items():
        full = DH.d64(prm.grad).reshape(-1)
        close(f'{mode} grad/{k}', full[torch.from_numpy(fx['idx/grad/' + k]).long()], torch.from_numpy(fx[f'{mode}/grad/{k}']).double(), full)
        within(f'{mode} grad/{k} float64', prm.grad, *bw['grads'][k])
        close(f'{mode} grad/{k} float64', prm.grad, bw['grads'][k][0])
    sd = m.state_dict()
    for l, p in enumerate(DH.prefixes(0)):
        got = DH.d64(sd[p + 'weight_u'])
        want = torch.from_numpy(fx[f'{mode}/u{l}']).double()
        assert float((got - want).abs().max()) <= CLOSE_UNIT, l
        if mode == 'eval':                                      # no iteration: the buffers are the loaded ones, bit for bit
            assert torch.equal(got, state[p + 'weight_u'].double()), l
            assert torch.equal(DH.d64(sd[p + 'weight_v']), state[p + 'weight_v'].double()), l
        else:
            sp = fw['g'][0]['w']['sp'][l]                       # the second call's buffers
            assert bool(((got - sp['u']).abs() <= sp['e_u'] + DH.U).all()), l
            assert float((DH.d64(sd[p + 'weight_v']) - sp['v']).abs().max()) <= CLOSE_UNIT, l


def test_the_pair_path_equals_two_calls(inputs):
    """the module runs d(y) and d(y_hat) as one batch where the weights do not move between them; the reference makes two calls: same bits"""
    state, y, y_hat = inputs
    m = _module(state, False)
    with torch.no_grad():
        rs, gs, frs, fgs = m(y.to(DEV), y_hat.to(DEV))
        ya, yb = y.to(DEV), y_hat.to(DEV)
        for i, d in enumerate(m.discriminators):
            if i:
                ya, yb = m.meanpools[i - 1](ya), m.meanpools[i - 1](yb)
            r, fr = d(ya)
            g, fg = d(yb)
            assert torch.equal(r, rs[i]) and torch.equal(g, gs[i])
            for l in range(N):
                assert torch.equal(fr[l], frs[i][l]) and torch.equal(fg[l], fgs[i][l])
    # train(): discriminators 1 and 2 still run as a pair, discriminator 0 as two calls whose weights differ
    mt = _module(state, True)
    with torch.no_grad():
        rs2, gs2, frs2, fgs2 = mt(y.to(DEV), y_hat.to(DEV))
    for i in (1, 2):
        assert torch.equal(rs2[i], rs[i]) and torch.equal(gs2[i], gs[i])
    assert not torch.equal(rs2[0], rs[0])


# ---- the step ----------------------------------------------------------------------------------------------------------------------------------------
def test_training_step_against_both_discriminators():
    from diffsinger_amd import (HifiGanMelLoss, MultiPeriodDiscriminator, MultiScaleDiscriminator, hifigan_adversarial_losses,
                                hifigan_discriminator_losses, hifigan_generator_losses, hifigan_training_step)
    from diffsinger_amd.vocoder import HifiGanGenerator
    from tests import hifigan_train_helpers as TH
    from tests import mel_loss_helpers as MH
    fxg = TH.fixture('plain')
    h = fxg['h']
    gen = HifiGanGenerator(h)
    gen.load_state_dict(fxg['state'], strict=True)
    gen = gen.to(DEV)
    B, T, hop = 2, 40, TH.hop_of(h)                             # tests/test_gpu_voc_optim.py's step
    crit = HifiGanMelLoss(dict(fft_size=256, hop_size=hop, win_size=256, audio_num_mel_bins=40, fmin=0, fmax=12000, audio_sample_rate=24000)).to(DEV)
    batch = dict(x=torch.randn(B, 80, T, generator=torch.Generator().manual_seed(71)).to(DEV), y=MH.signals('near', T * hop, B)[1][:, None].to(DEV))
    torch.manual_seed(5)
    mpd = MultiPeriodDiscriminator().to(DEV)
    msd = MultiScaleDiscriminator()
    msd.load_state_dict(SH.fixture_inputs()[0], strict=True)
    msd = msd.to(DEV).train()
    mpd2, msd2 = copy.deepcopy(mpd), copy.deepcopy(msd)
    u0 = {k: DH.d64(v) for k, v in msd.state_dict().items()}
    calls = [0]
    holders = list(msd.discriminators[0].convs) + [msd.discriminators[0].conv_post]
    versions = [m_.weight_u._version for m_ in holders]

    def count(*_):
        calls[0] += 1
    hook = msd.discriminators[0].register_forward_hook(count)
    out = hifigan_training_step(gen, [mpd, msd], crit, batch, dict(lambda_mel=45.0))
    hook.remove()
    assert len(out) == 9 and all(bool(torch.isfinite(v).all()) for v in out.values()), out
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for d in (mpd, msd) for p in d.parameters())
    # the two discriminators' terms, computed separately on copies in the step's order
    losses, y_hat = hifigan_generator_losses(gen, crit, batch['x'], None, batch['y'], lambda_mel=45.0)
    adv = [hifigan_adversarial_losses(d, batch['y'], y_hat) for d in (mpd2, msd2)]
    dis = [hifigan_discriminator_losses(d, batch['y'], y_hat) for d in (mpd2, msd2)]
    for name, got, want in (('gen_adv', out['gen_adv'], adv[0]['adv'] + adv[1]['adv']), ('gen_fm', out['gen_fm'], adv[0]['fm'] + adv[1]['fm']),
                            ('disc_real', out['disc_real'], dis[0][0] + dis[1][0]), ('disc_fake', out['disc_fake'], dis[0][1] + dis[1][1]),
                            ('disc_total', out['disc_total'], dis[0][0] + dis[1][0] + dis[0][1] + dis[1][1])):
        got, want = got.detach(), want.detach()
        rel = abs(float(got) - float(want)) / abs(float(want))
        print(f'{name}: {float(got):.6e}, relative difference {rel:.3e}')
        assert rel <= CLOSE_LOSS, (name, float(got), float(want))
    # the spectral buffers advanced once per d(.) call: four power iterations from the loaded state, in float64
    sd = msd.state_dict()
    for p in DH.prefixes(0):
        W, u, v = u0[p + 'weight_orig'].flatten(1), u0[p + 'weight_u'], u0[p + 'weight_v']
        us = [u]
        for _ in range(4):
            v = W.t() @ u
            v = v / v.norm()
            u = W @ v
            u = u / u.norm()
            us.append(u)
        got = DH.d64(sd[p + 'weight_u'])
        assert float((got - us[4]).abs().max()) <= CLOSE_UNIT, p
        assert torch.equal(sd[p + 'weight_u'], msd2.state_dict()[p + 'weight_u']), p
    assert calls == [4] and [m_.weight_u._version - v0_ for m_, v0_ in zip(holders, versions)] == [4] * 8       # one in-place update per call
