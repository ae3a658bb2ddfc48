"""GPU: the pooling of the HiFi-GAN multi-scale discriminator (include/dsv.h section "HiFi-GAN scale discriminator", csrc/hifigan_disc.hpp) through
the C ABI and through diffsinger_amd.hifigan_disc, against the float64 restatement of tests/hifigan_disc_helpers.py.

The comparison is the helpers' rule: |device - float64| <= bound element-wise, the bound built in float64 (three additions and an exact division
by 4: 4 u times the pooled absolute values), never from the code under test.  Tails [L, LS) of every padded output must be exactly zero."""
import pytest
import torch
import torch.nn.functional as F

from tests import hifigan_disc_helpers as DH

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')


def rnd(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def within(name, got, want, bound):
    err = (DH.d64(got) - want).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool(ok.all()), f'{name}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst error / bound {ratio:.3g}, max error {float(err.max()):.3g}'
    return ratio


@pytest.mark.parametrize('T', [2, 3, 4, 5, 1061])
def test_pooling_forward_and_backward(T):
    """against F.avg_pool1d in float64; T = 2, 3 -> 1, 4, 5 -> 2, 1061 -> 530 (more than one workgroup, an odd length, a tail)"""
    from diffsinger_amd import hifigan_disc as HD
    x = rnd(3, 1, T, seed=T)
    xd = x.to(DEV).requires_grad_(True)
    n0 = HD.launch_count()
    y = HD.avg_pool_op(xd)
    want, e = DH.pool_bound(x.double())
    assert torch.equal(want, F.avg_pool1d(x.double(), 4, 2, 1)) and y.shape == want.shape == (3, 1, T // 2)
    r1 = within('pool', y.detach(), want, e)
    g = rnd(3, 1, T // 2, seed=T + 1)
    y.backward(g.to(DEV))
    assert HD.launch_count() - n0 == 2                              # the docstring's arithmetic: 1 forward, 1 backward
    r2 = within('pool backward', xd.grad, *DH.pool_backward_bound(g.double(), None, T))
    y2 = HD.avg_pool_op(xd.detach())
    assert torch.equal(y2, y.detach())                              # two calls are bit-equal
    print(f'T={T}: worst error / bound {max(r1, r2):.3f}')


def test_pooling_tails_are_zero_and_bad_shapes_are_refused():
    from diffsinger_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    for L in (2, 33, 1061):
        LS, Lo = lib.dsv_padded_samples(L), L // 2
        LSo = lib.dsv_padded_samples(Lo)
        xc = rnd(2, L, seed=L)
        want = F.avg_pool1d(xc.double()[:, None], 4, 2, 1)[:, 0]
        # the rows as they lie: dense (ld = L), and a wider buffer whose columns beyond L hold NaN - nothing beyond sample L may be read
        for ld in (L, L + 5):
            x = torch.full((2, ld), NAN)
            x[:, :L] = xc
            x = x.to(DEV)
            out = torch.full((2, LSo), NAN, device=DEV)
            _lib.check(lib.dsv_hgd_avgpool(x.data_ptr(), out.data_ptr(), 2, L, ld, s))
            assert not bool(out[:, Lo:].ne(0).any()) and not bool(torch.isnan(out).any())
            within(f'pool L={L} ld={ld}', out[:, :Lo], want, 4 * DH.U * F.avg_pool1d(xc.double().abs()[:, None], 4, 2, 1)[:, 0])
        gc = rnd(2, Lo, seed=L + 1)
        first = None
        for ld in (Lo, Lo + 3):
            g = torch.full((2, ld), NAN)
            g[:, :Lo] = gc
            g = g.to(DEV)
            dx = torch.full((2, LS), NAN, device=DEV)
            _lib.check(lib.dsv_hgd_avgpool_backward(g.data_ptr(), dx.data_ptr(), 2, L, ld, s))
            assert not bool(dx[:, L:].ne(0).any()) and not bool(torch.isnan(dx).any())
            first = dx if first is None else first
            assert torch.equal(dx, first)
    x = torch.zeros(1, 64, device=DEV)
    assert lib.dsv_hgd_avgpool(x.data_ptr(), x.data_ptr() + 256, 1, 1, 1, s) == -1 and b'bad shape' in lib.dsd_last_error()
    assert lib.dsv_hgd_avgpool(x.data_ptr(), x.data_ptr() + 256, 1, 8, 7, s) == -1 and b'row stride' in lib.dsd_last_error()
    assert lib.dsv_hgd_avgpool(x.data_ptr(), x.data_ptr(), 1, 8, 8, s) == -1 and b'overlap' in lib.dsd_last_error()
    assert lib.dsv_hgd_avgpool(x.data_ptr(), x.data_ptr() + 16, 1, 8, 8, s) == -1 and b'overlap' in lib.dsd_last_error()        # partly overlapping
    assert lib.dsv_hgd_avgpool_backward(x.data_ptr() + 12, x.data_ptr(), 1, 8, 4, s) == -1 and b'overlap' in lib.dsd_last_error()
    assert lib.dsv_hgd_avgpool_backward(x.data_ptr(), x.data_ptr() + 256, 70000, 8, 4, s) == -1


def test_cumulative_pooling_and_cond_loss():
    """y -> pool -> pool as MultiScaleDiscriminator applies it, with a gradient through both; cond_discriminator_loss on LSGAN's operator"""
    from diffsinger_amd import hifigan_disc as HD
    x = rnd(2, 1, 301, seed=9)
    xd = x.to(DEV).requires_grad_(True)
    y = HD.avg_pool_op(HD.avg_pool_op(xd))
    p1, e1 = DH.pool_bound(x.double())
    p2, e2 = DH.pool_bound(p1, e1)
    assert y.shape == (2, 1, 75)
    within('pool o pool', y.detach(), p2, e2)
    outs = [y[:, 0], y[:, 0, :40] * 2.0]
    loss = HD.cond_discriminator_loss(outs)
    want = sum(DH.lsgan64(DH.d64(t), 0.0) for t in outs) / 2
    assert abs(float(loss) - float(want)) <= 16 * DH.U * float(want)
    loss.backward()
    g2 = (2.0 * p2 / p2.numel() + torch.cat([8.0 * p2[:, :, :40] / (2 * 40), torch.zeros(2, 1, 35, dtype=torch.float64)], 2)) / 2
    g1, eg1 = DH.pool_backward_bound(g2, 16 * DH.U * g2.abs() + 8 * e2 / 40, 150)
    within('d cond loss / dx', xd.grad, *DH.pool_backward_bound(g1, eg1, 301))
