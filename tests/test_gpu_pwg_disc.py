"""GPU: the ParallelWaveGAN discriminator (include/dsv.h section "PWG discriminator", csrc/pwg_disc.hpp) at operator level through the C ABI and
as a whole through diffsinger_amd.pwg_disc, against the float64 restatements of tests/pwg_disc_helpers.py.

Every comparison is the helpers' rule: |device - float64| <= 16 u sum|term|, element-wise, sum|term| computed in float64 from the DEVICE'S OWN
operands (u = 2^-24; where the abs-sum is 0 the result must be exactly 0).  The whole-module tests get the device's own operands of every step
by replaying forward and backward call by call through the C ABI (`Ops` below; the kernels are deterministic, so the replay is bit-identical
to what the autograd node computed - asserted) - a bound propagated through ten layers would be four orders wider than the errors it is
meant to catch.  Every test prints its measured maximum beside its bound."""
import pytest
import torch
import torch.nn.functional as F

from tests import pwg_disc_helpers as DH

pytestmark = pytest.mark.gpu

C = 64
DEV = 'cuda'


def rnd(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Ops:
    """The C ABI on torch tensors, test side (ctypes only - independent of diffsinger_amd.pwg_disc)."""

    def __init__(self):
        from diffsinger_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.tile, self.split = self.lib.dsv_pwgd_tile(), self.lib.dsv_pwgd_wgrad_split()

    def s(self):
        return torch.cuda.current_stream().cuda_stream

    def call(self, name, *args):
        self._lib.check(getattr(self.lib, name)(*args, self.s()), name)

    def ls(self, T):
        return self.lib.dsv_padded_samples(T)

    def padded(self, x):
        """[..., T] (CPU or device) -> device float32 [..., LS], zero tail"""
        return F.pad(x.to(DEV, torch.float32), (0, self.ls(x.shape[-1]) - x.shape[-1])).contiguous()

    def pack(self, mat):
        mat = mat.to(DEV, torch.float32).contiguous()
        buf = torch.empty(self.lib.dsv_packed_floats(mat.shape[0], mat.shape[1], 1), device=DEV)
        self.call('dsv_pack_weight', mat.data_ptr(), mat.shape[0], mat.shape[1], 1, buf.data_ptr())
        return buf

    def pack_fwd(self, w):
        return self.pack(w.permute(0, 2, 1).reshape(C, 3 * C))

    def pack_bwd(self, w):
        return self.pack(w.flip(2).permute(1, 2, 0).reshape(C, 3 * C))

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()

    def layer(self, inp, packed, bias, saved, T, dil, slope, backward):
        out = torch.full_like(inp, float('nan'))
        self.call('dsv_pwgd_layer', inp.data_ptr(), packed.data_ptr(), self.p(bias), self.p(saved), out.data_ptr(), inp.shape[0], T, dil, slope,
                  int(backward))
        return out

    def wgrad(self, G, a, T, dil, want_db=True, ws=None):
        B = G.shape[0]
        if ws is None:
            ws = torch.empty(self.lib.dsv_pwgd_wgrad_workspace_floats(B, T), device=DEV)
        dw = torch.full((C, C, 3), float('nan'), device=DEV)
        db = torch.full((C,), float('nan'), device=DEV) if want_db else None
        self.call('dsv_pwgd_wgrad', G.data_ptr(), a.data_ptr(), ws.data_ptr(), dw.data_ptr(), self.p(db), B, T, dil)
        return dw, db

    def edge_ws(self, B, T):
        return torch.empty(self.lib.dsv_pwgd_edge_workspace_floats(B, T), device=DEV)

    def first(self, xp, w, b, T, slope):
        out = torch.full((xp.shape[0], C, xp.shape[-1]), float('nan'), device=DEV)
        self.call('dsv_pwgd_first', xp.data_ptr(), w.data_ptr(), self.p(b), out.data_ptr(), xp.shape[0], T, slope)
        return out

    def first_backward(self, g0, xp, w, T, want_db=True, want_dx=True):
        B = g0.shape[0]
        dw = torch.full((C, 1, 3), float('nan'), device=DEV)
        db = torch.full((C,), float('nan'), device=DEV) if want_db else None
        dx = torch.full((B, g0.shape[-1]), float('nan'), device=DEV) if want_dx else None
        self.call('dsv_pwgd_first_backward', g0.data_ptr(), xp.data_ptr(), w.data_ptr(), self.edge_ws(B, T).data_ptr(), dw.data_ptr(), self.p(db),
                  self.p(dx), B, T)
        return dw, db, dx

    def last(self, a, w, b, T):
        out = torch.full((a.shape[0], a.shape[-1]), float('nan'), device=DEV)
        self.call('dsv_pwgd_last', a.data_ptr(), w.data_ptr(), self.p(b), out.data_ptr(), a.shape[0], T)
        return out

    def last_backward(self, gp, a, w, T, slope, want_db=True):
        B = a.shape[0]
        dw = torch.full((1, C, 3), float('nan'), device=DEV)
        db = torch.full((1,), float('nan'), device=DEV) if want_db else None
        ga = torch.full_like(a, float('nan'))
        self.call('dsv_pwgd_last_backward', gp.data_ptr(), a.data_ptr(), w.data_ptr(), self.edge_ws(B, T).data_ptr(), dw.data_ptr(), self.p(db),
                  ga.data_ptr(), B, T, slope)
        return dw, db, ga


@pytest.fixture(scope='module')
def ops():
    return Ops()


def within(name, got, want, bound, T=None):
    """assert |got - want| <= bound element-wise (got: device tensor, possibly LS-padded: the tail must be exactly 0); print the figures"""
    got = DH.d64(got)
    if T is not None:
        assert bool((got[..., T:] == 0).all()), f'{name}: [T, LS) is not zero'
        got = got[..., :T]
    got = got.reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f'{name}: not finite (an element was not written)'
    err = (got - want).abs()
    k = int((err - bound).argmax())
    ratio = float((err / bound.clamp_min(1e-300)).max()) * 16.0
    print(f'{name}: max err {float(err.max()):.3e}; tightest element err {float(err.flatten()[k]):.3e} <= bound {float(bound.flatten()[k]):.3e}; '
          f'max err / (u sum|term|) {ratio:.2f} (bound 16)')
    assert bool((err <= bound).all()), name
    zero = bound == 0
    if bool(zero.any()):
        assert bool((got[zero] == 0).all()), f'{name}: not exactly 0 where the abs-sum is 0'


def layer_shapes(t):
    return [(1, 1, 1), (2, 7, 8), (2, t - 1, 3), (2, t, 3), (2, t + 1, 3), (2, 2 * t + 37, 8), (2, 1061, 5)]


def shape_id(v):
    return 'x'.join(str(i) for i in v)


# the tile is a constant of the library: 128 (asserted in the tests, so a change of the tile fails loudly instead of missing the edges)
TILE, SPLIT = 128, 256


# ---- 1. layer forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', layer_shapes(TILE), ids=shape_id)
def test_layer_forward(ops, shape):
    assert ops.tile == TILE
    B, T, dil = shape
    slope = 0.2
    x, w, b = rnd(B, C, T, seed=1), rnd(C, C, 3, seed=2, scale=0.1), rnd(C, seed=3, scale=0.1)
    xp, wp, bd = ops.padded(x), ops.pack_fwd(w), b.to(DEV)
    out = ops.layer(xp, wp, bd, None, T, dil, slope, False)
    pre, bound = DH.conv_bound(DH.d64(xp)[..., :T], w.double(), b.double(), dil)
    want = DH.leaky(pre, slope)
    within(f'layer forward {shape}', out, want, bound + DH.U * want.abs(), T)
    if B > 1:                                                   # batch rows are independent: swapped input rows give swapped output rows, bit for bit
        out2 = ops.layer(xp.flip(0).contiguous(), wp, bd, None, T, dil, slope, False)
        assert torch.equal(out2, out.flip(0))
        assert not torch.equal(out[0], out[1])
    out_nb = ops.layer(xp, wp, None, None, T, dil, slope, False)  # no bias
    pre, bound = DH.conv_bound(DH.d64(xp)[..., :T], w.double(), None, dil)
    within(f'layer forward {shape} without bias', out_nb, DH.leaky(pre, slope), bound + DH.U * pre.abs(), T)


# ---- 2. layer data gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', layer_shapes(TILE), ids=shape_id)
def test_layer_data_gradient(ops, shape):
    B, T, dil = shape
    slope = 0.2
    G, w = rnd(B, C, T, seed=4), rnd(C, C, 3, seed=5, scale=0.1)
    saved = rnd(B, C, T, seed=6)
    saved[torch.rand(B, C, T, generator=torch.Generator().manual_seed(7)) < 0.15] = 0.0         # exact zeros beside both signs
    saved[0, 0, 0] = 0.0
    Gp, sp = ops.padded(G), ops.padded(saved)
    out = ops.layer(Gp, ops.pack_bwd(w), None, sp, T, dil, slope, True)
    y, bound = DH.dgrad_bound(G.double(), None, w.double(), dil)
    m = DH.mask_of(saved.double(), slope)
    assert bool((m[saved == 0] == slope).all()) and bool((saved > 0).any() or T == 1) and bool((saved == 0).any())
    within(f'layer data gradient {shape}', out, y * m, bound * m + DH.U * (y * m).abs(), T)
    z = saved == 0                                              # an output of exactly 0 takes the slope: nowhere near the unmasked value
    if bool((y[z].abs() > 100 * bound[z]).any()):
        got = DH.d64(out)[..., :T][z]
        assert bool(((got - y[z]).abs() > bound[z])[y[z].abs() > 100 * bound[z]].all())
    plain = ops.layer(Gp, ops.pack_bwd(w), None, None, T, dil, slope, True)                       # saved NULL: no mask
    within(f'layer data gradient {shape} without mask', plain, y, bound, T)


# ---- 3. weight and bias gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dil', [1, 8])
@pytest.mark.parametrize('T', [7, SPLIT - 1, SPLIT + 1, 2 * SPLIT + 37])
def test_weight_and_bias_gradient(ops, T, dil):
    assert ops.split == SPLIT
    B = 2
    G, a = rnd(B, C, T, seed=8), rnd(B, C, T, seed=9)
    Gp, ap = ops.padded(G), ops.padded(a)
    n = ops.lib.dsv_pwgd_wgrad_workspace_floats(B, T)
    assert n == B * ((T + SPLIT - 1) // SPLIT) * (C * C * 3 + C)
    ws = torch.full((n + 4096,), -7.0, device=DEV)              # the declared size and a guard behind it
    dw, db = ops.wgrad(Gp, ap, T, dil, ws=ws)
    assert bool((ws[n:] == -7.0).all()), 'the workspace is larger than declared'
    (wv, wb), (bv, bb) = DH.wgrad_bound(G.double(), None, a.double(), None, dil)
    within(f'dW T={T} dil={dil}', dw, wv, wb)
    within(f'db T={T} dil={dil}', db, bv, bb)
    if T <= dil:                                                # every outer tap falls off both ends: exactly 0 (checked by `within` where the abs-sum is 0)
        assert bool((wb[:, :, 0] == 0).all()) and bool((wb[:, :, 2] == 0).all()) and bool((dw[:, :, 0] == 0).all()) and bool((dw[:, :, 2] == 0).all())
    dw2, db2 = ops.wgrad(Gp, ap, T, dil)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dw3, none = ops.wgrad(Gp, ap, T, dil, want_db=False)
    assert none is None and torch.equal(dw, dw3)


# ---- 4. first and last layers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, TILE + 1])
def test_first_and_last_layers(ops, T):
    B, slope = 2, 0.2
    x, w0, b0 = rnd(B, 1, T, seed=10), rnd(C, 1, 3, seed=11, scale=0.6), rnd(C, seed=12, scale=0.1)
    xp = ops.padded(x[:, 0])
    a0 = ops.first(xp, w0.to(DEV), b0.to(DEV), T, slope)
    pre, bound = DH.conv_bound(x.double(), w0.double(), b0.double(), 1)
    within(f'first forward T={T}', a0, DH.leaky(pre, slope), bound + DH.U * pre.abs(), T)
    g0 = rnd(B, C, T, seed=13)
    dw, db, dx = ops.first_backward(ops.padded(g0), xp, w0.to(DEV), T)
    (wv, wb), (bv, bb) = DH.wgrad_bound(g0.double(), None, x.double(), None, 1)
    within(f'first dW T={T}', dw, wv, wb)
    within(f'first db T={T}', db, bv, bb)
    dv, dbnd = DH.dgrad_bound(g0.double(), None, w0.double(), 1)
    within(f'first dx T={T}', dx, dv[:, 0], dbnd[:, 0], T)
    dw2, none, none2 = ops.first_backward(ops.padded(g0), xp, w0.to(DEV), T, want_db=False, want_dx=False)
    assert none is None and none2 is None and torch.equal(dw, dw2)
    a, wl, bl = rnd(B, C, T, seed=14), rnd(1, C, 3, seed=15, scale=0.1), rnd(1, seed=16)
    a[torch.rand(B, C, T, generator=torch.Generator().manual_seed(17)) < 0.15] = 0.0
    ap = ops.padded(a)
    p = ops.last(ap, wl.to(DEV), bl.to(DEV), T)
    pv, pb = DH.conv_bound(a.double(), wl.double(), bl.double(), 1)
    within(f'last forward T={T}', p, pv[:, 0], pb[:, 0], T)
    gp = rnd(B, 1, T, seed=18)
    dw, db, ga = ops.last_backward(ops.padded(gp[:, 0]), ap, wl.to(DEV), T, slope)
    (wv, wb), (bv, bb) = DH.wgrad_bound(gp.double(), None, a.double(), None, 1)
    within(f'last dW T={T}', dw, wv, wb)
    within(f'last db T={T}', db, bv, bb)
    gv, gb = DH.dgrad_bound(gp.double(), None, wl.double(), 1)
    m = DH.mask_of(a.double(), slope)
    within(f'last data gradient T={T}', ga, gv * m, gb * m + DH.U * (gv * m).abs(), T)


def test_dx_is_computed_only_when_x_requires_grad():
    from diffsinger_amd import pwg_disc as PD
    ws, bs = device_params(DH.synth_state(DH.module_shapes(3, True, False), 5), 3, grad=True)
    x = rnd(2, 1, 40, seed=19).to(DEV)
    counts = []
    for need in (False, True):
        xi = x.clone().requires_grad_(need)
        n0 = PD.launch_count()
        PD.generator_loss([PD.pwg_disc_op(xi, ws, bs, 0.2)]).backward()
        counts.append(PD.launch_count() - n0)
        assert (xi.grad is not None) == need
    print(f'launches of forward + generator_loss + backward, 3 layers: {counts[0]} without dx, {counts[1]} with')
    assert counts[1] == counts[0] + 1
    assert counts[0] == (3 + 3) + 3 + 3 * 3                     # forward n + 3, loss 2 + 1, backward 3 n (diffsinger_amd/pwg_disc.py)


# ---- whole module --------------------------------------------------------------------------------------------------------------------------
def device_params(state, n, grad=False):
    """plain float32 weights / biases on the device from a state dict in either form"""
    ws64, bs64 = DH.plain_params(state, n)
    ws = [w.float().to(DEV).requires_grad_(grad) for w in ws64]
    bs = [None if b is None else b.float().to(DEV).requires_grad_(grad) for b in bs64]
    return ws, bs


def check_network(ops, name, x, ws, bs, slope, flips=True):
    """pwg_disc_op forward + generator_loss + backward on plain device weights (leaves), every step against float64 from the device's own
    operands.  -> dict(p, acts, dx, dw, db) (device tensors)"""
    from diffsinger_amd import pwg_disc as PD
    n = len(ws)
    B, _, T = x.shape
    xg = x.clone().requires_grad_(True)
    p, acts = PD.pwg_disc_op(xg, ws, bs, slope, return_saved=True)
    assert tuple(p.shape) == (B, 1, T) and all(tuple(a.shape) == (B, C, T) for a in acts) and len(acts) == n - 1
    PD.generator_loss([p]).backward()
    w64, b64 = [DH.d64(w) for w in ws], [None if b is None else DH.d64(b) for b in bs]
    x64, a64 = DH.d64(x), [DH.d64(a) for a in acts]
    # forward: every layer from the device's own input
    f = DH.forward64(x64, w64, b64, slope, inputs=a64)
    for i in range(n - 1):
        within(f'{name}: activation {i}', acts[i], f['act'][i], f['e_act'][i])
    within(f'{name}: output', p, f['p'], f['e_p'])
    if flips:
        # signs against the pure float64 forward (own masks, bound propagated from x): they may differ only where the float64 pre-activation
        # is within its bound of 0, and on at most 1e-5 of the elements
        own = DH.forward64(x64, w64, b64, slope)
        nflip = total = 0
        for i in range(n - 1):
            d = (a64[i] > 0) != (own['pre'][i] > 0)
            assert bool((own['pre'][i].abs()[d] <= own['e_act'][i][d]).all()), f'{name}: a sign of layer {i} differs away from 0'
            nflip, total = nflip + int(d.sum()), total + d.numel()
        print(f'{name}: {nflip} of {total} activation signs differ from the float64 forward (bound {1e-5 * total:.1f})')
        assert nflip <= 1e-5 * total
    # backward: replayed call by call through the C ABI, so that every step's device operands are at hand
    pl = p.detach().clone().requires_grad_(True)
    PD.generator_loss([pl]).backward()
    gp = pl.grad                                                 # [B][1][T] on the device
    gpv, gpb = DH.generator_gp(DH.d64(p), None)
    within(f'{name}: d loss / d p', gp, gpv, gpb)
    gpp, ap = ops.padded(gp[:, 0]), [ops.padded(a.detach()) for a in acts]
    dws, dbs = [None] * n, [None] * n
    dws[n - 1], dbs[n - 1], G = ops.last_backward(gpp, ap[n - 2], ws[n - 1].detach(), T, slope, bs[n - 1] is not None)
    gp64 = DH.d64(gp)
    (wv, wb), (bv, bb) = DH.wgrad_bound(gp64, None, a64[n - 2], None, 1)
    within(f'{name}: dW {n - 1}', dws[n - 1], wv, wb)
    if bs[n - 1] is not None:
        within(f'{name}: db {n - 1}', dbs[n - 1], bv, bb)
    gv, gb = DH.dgrad_bound(gp64, None, w64[n - 1], 1)
    m = DH.mask_of(a64[n - 2], slope)
    within(f'{name}: G {n - 2}', G, gv * m, gb * m + DH.U * (gv * m).abs(), T)
    for l in range(n - 2, 0, -1):
        G64 = DH.d64(G)[..., :T]
        dws[l], dbs[l] = ops.wgrad(G, ap[l - 1], T, l, bs[l] is not None)
        (wv, wb), (bv, bb) = DH.wgrad_bound(G64, None, a64[l - 1], None, l)
        within(f'{name}: dW {l}', dws[l], wv, wb)
        if bs[l] is not None:
            within(f'{name}: db {l}', dbs[l], bv, bb)
        G = ops.layer(G, ops.pack_bwd(ws[l].detach()), None, ap[l - 1], T, l, slope, True)
        gv, gb = DH.dgrad_bound(G64, None, w64[l], l)
        m = DH.mask_of(a64[l - 1], slope)
        within(f'{name}: G {l - 1}', G, gv * m, gb * m + DH.U * (gv * m).abs(), T)
    G64 = DH.d64(G)[..., :T]
    dws[0], dbs[0], dx = ops.first_backward(G, ops.padded(x[:, 0]), ws[0].detach(), T, bs[0] is not None)
    (wv, wb), (bv, bb) = DH.wgrad_bound(G64, None, x64, None, 1)
    within(f'{name}: dW 0', dws[0], wv, wb)
    if bs[0] is not None:
        within(f'{name}: db 0', dbs[0], bv, bb)
    dv, dbnd = DH.dgrad_bound(G64, None, w64[0], 1)
    within(f'{name}: dx', dx, dv[:, 0], dbnd[:, 0], T)
    # ... and the replay IS what the autograd node computed
    assert torch.equal(xg.grad, dx[:, None, :T]), f'{name}: dx of the autograd node differs from the replay'
    for i in range(n):
        assert torch.equal(ws[i].grad, dws[i]), f'{name}: dW {i} of the autograd node differs from the replay'
        assert (bs[i] is None) or torch.equal(bs[i].grad, dbs[i]), f'{name}: db {i} of the autograd node differs from the replay'
    return dict(p=p.detach(), acts=[a.detach() for a in acts], dx=xg.grad, dw=[w.grad for w in ws], db=[None if b is None else b.grad for b in bs])


def test_whole_module_ten_layers_against_float64(ops):
    n, slope = 10, 0.2
    ws, bs = device_params(DH.synth_state(DH.module_shapes(n), 11), n, grad=True)
    x = rnd(2, 1, 1061, seed=20).to(DEV)
    r = check_network(ops, '10 layers', x, ws, bs, slope)
    assert float(r['p'].abs().max()) > 0.1 and all(float(a.abs().mean()) > 0.05 for a in r['acts'])        # the seeded state keeps the stack alive


def test_whole_module_against_the_reference_fixture(ops):
    """layers = 4: the module with the fixture's state against the reference's float32 CPU numbers - per tensor within twice the fixture's own
    distance from float64 plus the rule's bound of the tensor's last operation (float64 operands)."""
    from diffsinger_amd import ParallelWaveGANDiscriminator, generator_loss
    fx = DH.fixture()
    n, slope = fx['layers'], fx['slope']
    m = ParallelWaveGANDiscriminator(layers=n)
    m.load_state_dict(fx['state'], strict=True)
    m = m.to(DEV)
    x = fx['x'].to(DEV).requires_grad_(True)
    p = m(x)
    generator_loss([p]).backward()
    # float64, own masks
    w64, b64 = DH.plain_params(fx['state'], n)
    x64 = DH.d64(fx['x'])
    f = DH.forward64(x64, w64, b64, slope)
    gp, _ = DH.generator_gp(f['p'], None)
    bw = DH.backward64(gp, None, x64, w64, f['act'], slope)
    rows = [('out', p, fx['out'], f['p'], DH.conv_bound(f['act'][n - 2], w64[n - 1], b64[n - 1], 1)[1]), ('dx', x.grad, fx['dx'], *bw['dx'])]
    for i in range(n):
        pre = f'conv_layers.{2 * i}.'
        conv = m.conv_layers[2 * i]
        (gg, bg), (gv, bv) = DH.weight_norm_grads64(DH.d64(fx['state'][pre + 'weight_g']), DH.d64(fx['state'][pre + 'weight_v']), *bw['dw'][i])
        rows += [(pre + 'weight_g', conv.weight_g.grad, fx['grads'][pre + 'weight_g'], gg, bg),
                 (pre + 'weight_v', conv.weight_v.grad, fx['grads'][pre + 'weight_v'], gv, bv),
                 (pre + 'bias', conv.bias.grad, fx['grads'][pre + 'bias'], *bw['db'][i])]
    for name, got, ref32, want64, bound in rows:
        dist = float((DH.d64(ref32) - want64).abs().max())
        err = (DH.d64(got) - DH.d64(ref32)).abs()
        tol = 2.0 * dist + bound
        k = int((err - tol).argmax())
        print(f'{name}: fixture vs float64 {dist:.3e}; device vs fixture max {float(err.max()):.3e}, tightest element {float(err.flatten()[k]):.3e} <= '
              f'{float(tol.flatten()[k]):.3e}')
        assert bool((err <= tol).all()), name
    # the same network on plain weights, every step from the device's own operands
    ws, bs = device_params(fx['state'], n, grad=True)
    r = check_network(ops, 'fixture state, 4 layers', fx['x'].to(DEV), ws, bs, slope)
    assert float((r['p'] - p.detach()).abs().max()) <= 1e-4      # the module's own g v / ||v|| (float32 on the device) against the float64 one, rounded


# ---- 6. variants ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['bias=False', 'use_weight_norm=False', 'layers=3', 'negative_slope=0.1', 'remove_weight_norm', 'offset view'])
def test_variants(ops, variant):
    from diffsinger_amd import ParallelWaveGANDiscriminator, generator_loss
    kw = dict(layers=5)
    if variant == 'bias=False':
        kw['bias'] = False
    elif variant == 'use_weight_norm=False':
        kw['use_weight_norm'] = False
    elif variant == 'layers=3':
        kw['layers'] = 3
    elif variant == 'negative_slope=0.1':
        kw['nonlinear_activation_params'] = {'negative_slope': 0.1}
    n = kw['layers']
    slope = kw.get('nonlinear_activation_params', {'negative_slope': 0.2})['negative_slope']
    m = ParallelWaveGANDiscriminator(**kw)
    m.load_state_dict(DH.synth_state(DH.module_shapes(n, kw.get('bias', True), kw.get('use_weight_norm', True)), 21, slope), strict=True)
    if variant == 'remove_weight_norm':
        m.remove_weight_norm()
        assert all(k.endswith('.weight') or k.endswith('.bias') for k in m.state_dict())
    m = m.to(DEV)
    x = rnd(2, 1, 97, seed=22).to(DEV)
    if variant == 'offset view':                                # a 4-byte-offset, non-contiguous view
        big = torch.zeros(2, 1, 98, device=DEV)
        big[:, :, 1:] = x
        big.requires_grad_(True)
        xin = big[:, :, 1:]
        assert not xin.is_contiguous() and xin.data_ptr() % 16 == 4
    else:
        xin = x.clone().requires_grad_(True)
    p = m(xin)
    generator_loss([p]).backward()
    # the module is pwg_disc_op on its plain weights: bit for bit, and that against float64
    convs = [m.conv_layers[2 * i] for i in range(n)]
    with torch.no_grad():
        ws = [(torch._weight_norm(c.weight_v, c.weight_g, 0) if hasattr(c, 'weight_g') else c.weight).clone() for c in convs]
        bs = [None if c.bias is None else c.bias.clone() for c in convs]
    for t in ws + [b for b in bs if b is not None]:
        t.requires_grad_(True)
    r = check_network(ops, variant, x, ws, bs, slope, flips=False)
    assert torch.equal(p.detach(), r['p'])
    dx = big.grad[:, :, 1:] if variant == 'offset view' else xin.grad
    assert torch.equal(dx, r['dx'])
    if variant == 'offset view':
        assert bool((big.grad[:, :, 0] == 0).all())
    for i, c in enumerate(convs):
        if c.bias is not None:
            assert torch.equal(c.bias.grad, r['db'][i])
        if not hasattr(c, 'weight_g'):
            assert torch.equal(c.weight.grad, r['dw'][i])


# ---- 7. weight-norm gradients --------------------------------------------------------------------------------------------------------------
def test_weight_norm_gradients(ops):
    from diffsinger_amd import ParallelWaveGANDiscriminator, generator_loss, pwg_disc_op
    n = 4
    m = ParallelWaveGANDiscriminator(layers=n)
    m.load_state_dict(DH.synth_state(DH.module_shapes(n), 23), strict=True)
    m = m.to(DEV)
    x = rnd(2, 1, 97, seed=24).to(DEV)
    generator_loss([m(x)]).backward()
    convs = [m.conv_layers[2 * i] for i in range(n)]
    with torch.no_grad():
        ws = [torch._weight_norm(c.weight_v, c.weight_g, 0).clone().requires_grad_(True) for c in convs]
    generator_loss([pwg_disc_op(x, ws, [c.bias.detach() for c in convs], 0.2)]).backward()
    for i, c in enumerate(convs):
        (gg, bg), (gv, bv) = DH.weight_norm_grads64(DH.d64(c.weight_g), DH.d64(c.weight_v), DH.d64(ws[i].grad))
        within(f'weight_g.grad {i}', c.weight_g.grad, gg, bg)
        within(f'weight_v.grad {i}', c.weight_v.grad, gv, bv)


# ---- 8. LSGAN ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('target', [0.0, 1.0])
@pytest.mark.parametrize('n', [1, 255, 256 * 3 + 5])
def test_lsgan_loss_and_gradient(n, target):
    from diffsinger_amd import lsgan_loss_op
    d = (rnd(n, seed=25) + 0.3).to(DEV).requires_grad_(True)
    loss = lsgan_loss_op(d, target)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    want, got = float(DH.lsgan64(d, target)), float(loss.detach())
    print(f'lsgan n={n} target={target}: loss {got:.9g}, float64 {want:.9g}, |diff| {abs(got - want):.3e} <= {4 * DH.U * want:.3e}')
    assert abs(got - want) <= 4 * DH.U * want
    g = 0.37
    (loss * g).backward()
    g32 = float(torch.tensor(g, dtype=torch.float32))
    gw = 2.0 * (DH.d64(d) - target) / n * g32
    err = (DH.d64(d.grad) - gw).abs()
    print(f'lsgan gradient n={n}: max err / |value| {float((err / gw.abs().clamp_min(1e-300)).max()) / DH.U:.2f} u (bound 4 u)')
    assert bool((err <= 4 * DH.U * gw.abs()).all())


def test_generator_and_discriminator_loss_on_lists():
    from diffsinger_amd import discriminator_loss, generator_loss
    real = [rnd(2, 1, t, seed=26 + i).to(DEV) + 0.8 for i, t in enumerate((31, 500, 1061))]
    fake = [rnd(2, 1, t, seed=36 + i).to(DEV) for i, t in enumerate((31, 500, 1061))]
    gl = generator_loss(fake)
    rl, fl = discriminator_loss(real, fake)
    want_g = sum(float(((1 - DH.d64(t)) ** 2).mean()) for t in fake) / 3
    want_r = sum(float(((1 - DH.d64(t)) ** 2).mean()) for t in real) / 3
    want_f = sum(float((DH.d64(t) ** 2).mean()) for t in fake) / 3
    for name, got, want in (('generator_loss', gl, want_g), ('discriminator_loss real', rl, want_r), ('discriminator_loss generated', fl, want_f)):
        print(f'{name}: {float(got):.9g}, float64 {want:.9g}, |diff| {abs(float(got) - want):.3e} <= {8 * DH.U * want:.3e}')
        assert abs(float(got) - want) <= 8 * DH.U * want        # 4 u per term, two more float32 additions and a division


# ---- 9. determinism and capture ------------------------------------------------------------------------------------------------------------
def test_determinism_and_graph_capture():
    from diffsinger_amd import ParallelWaveGANDiscriminator, generator_loss
    n = 10
    m = ParallelWaveGANDiscriminator(layers=n)
    m.load_state_dict(DH.synth_state(DH.module_shapes(n), 27), strict=True)
    m = m.to(DEV)
    params = list(m.parameters())
    x = rnd(2, 1, 700, seed=28).to(DEV).requires_grad_(True)

    def step():
        p = m(x)
        loss = generator_loss([p])
        grads = torch.autograd.grad(loss, [x] + params)
        return [p, loss] + list(grads)

    a = [t.detach().clone() for t in step()]
    b = [t.detach().clone() for t in step()]
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # raises on a synchronisation inside the region
        outs = step()
    for _ in range(2):
        for t in outs:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v.detach()) for u, v in zip(a, outs))


# ---- 10. validation ------------------------------------------------------------------------------------------------------------------------
def test_validation():
    from diffsinger_amd import ParallelWaveGANDiscriminator, generator_loss
    m = ParallelWaveGANDiscriminator(layers=3).to(DEV)
    for bad in (torch.zeros(2, 1, 8), torch.zeros(2, 1, 8, dtype=torch.float64, device=DEV), torch.zeros(2, 2, 8, device=DEV),
                torch.zeros(2, 8, device=DEV), torch.zeros(2, 1, 0, device=DEV)):
        with pytest.raises(ValueError, match='x must be'):
            m(bad)
    p = m(torch.zeros(2, 1, 8, device=DEV))
    loss = generator_loss([p])
    loss.backward()
    with pytest.raises(RuntimeError):
        generator_loss([p]).backward()                          # a second backward through the output: the saved activations are gone
