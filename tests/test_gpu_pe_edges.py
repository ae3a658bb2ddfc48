"""GPU: the PitchExtractor's norms and pitch loss at the sizes a training step has (usr/configs/midi/pe.yaml: max_tokens 20000, max_frames 8000)
and at the edges of their kernels: k_pe_bn_train on both sides of its LDS stage (kPeBnStage4) and unstaged at 20 000 frames, k_pe_bn_train_bwd,
k_fs_group_norm / k_pe_gn_bwd at long frame counts and at 1, 3 and 64 (kPeGnMaxCg) channels per group, k_pe_f0_partial / k_pe_f0_bwd past the
sizes where their grids start to stride, k_fs_affine past the cap of ew_grid, and the flags no other test sets (keep=None,
track_running_stats=False, relu=False without residual, T == TS, a third pitch_pred channel).

Yardsticks and bound: tests/pe_edge_helpers.py - float64 aten / pe_train_helpers.f0_losses; the error (pe_train_helpers.rel_err) is at most
pe_train_helpers.bound (4 x, floor 2e-6) of the error of the elementary float32 restatement of the same operator on the same inputs.  Every
element of every tensor is compared; the inputs keep every ReLU input away from its kink (tests/test_pe_edges_host.py asserts that, and that the
bound catches the bugs these shapes are for).

What these tests found: k_fs_group_norm and k_pe_gn_bwd summed x itself, so on x = 100 + 0.1 N(0,1) at 1 x 16 x 8000 (one group of 128 000
values) y was 1.516e-05 off float64 against a bound of 4.458e-06 (3.4 x; the float32 restatement is 1.115e-06 off).  Both kernels now keep the
mean as pivot + dm (pivot = the group's first value) and centre x as (x - pivot) - dm: 9.6e-08 on the same case."""
import pytest
import torch

from tests import pe_edge_helpers as E
from tests.test_gpu_pe import _build, _compare

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _cm(x_bct):
    """[B,C,T] on the CPU -> channel-major [B][C][TS] on the device."""
    from diffsinger_amd.fs2 import to_cm
    return to_cm(x_bct.transpose(1, 2).to(DEV))


def _bct(x_cm, T):
    from diffsinger_amd.fs2 import from_cm
    return from_cm(x_cm, T).transpose(1, 2).cpu()


def _zero_tail(*tensors, T):
    return all(float(t.detach()[:, :, T:].abs().sum()) == 0.0 for t in tensors)


# ---------------------------------------------------------------------------------------------------------------------
# 1. BatchNorm on batch statistics, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
BN_CASES = [(B, T, kind, 8, True, True) for B, T in E.BN_SHAPES for kind in E.BN_KINDS] + [
    (10, 2000, 'kink_free', 8, False, True),         # keep=None
    (10, 2000, 'kink_free', 8, True, False),         # BatchNorm1d(track_running_stats=False): null running pointers
    (8, 1025, 'kink_free', 64, True, True)]          # a grid of 64 channels


@pytest.mark.parametrize('B,T,kind,C,masked,track', BN_CASES)
def test_batch_norm_train_at_training_size(B, T, kind, C, masked, track):
    from diffsinger_amd import pe
    c, want, ref = E.bn_refs(B, T, kind, C, masked)
    relu_in = c['relu_in']
    assert E.bn_staged(B, T) == ((B, T) in [(8, 1024), (1, 8192)])

    def module():
        bn = torch.nn.BatchNorm1d(C, track_running_stats=track).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(c['gamma']); bn.bias.copy_(c['beta'])
            if track:
                bn.running_mean.copy_(c['rm']); bn.running_var.copy_(c['rv'])
        return bn
    bn = module()
    kd = c['keep'].to(DEV).contiguous() if masked else None
    xc, dyc = _cm(c['x']).requires_grad_(True), _cm(c['dy'])
    assert xc.shape[2] == E.fs_ts(T)
    y = pe.batch_norm_train_cm(xc, T, bn, relu_in=relu_in, keep=kd)
    y.backward(dyc)
    assert _zero_tail(y, xc.grad, T=T)
    if track:
        assert int(bn.num_batches_tracked) == 1
        rm2, rv2 = c['rm'].to(DEV), c['rv'].to(DEV)
    else:
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
        rm2 = rv2 = None
    # the statistics, and a second run: bit for bit the same
    y2, mean, rstd = pe._batch_norm_train_raw(xc.detach(), T, bn.weight.detach(), bn.bias.detach(), rm2, rv2, bn.eps, bn.momentum, relu_in, kd)
    assert torch.equal(y2, y.detach())
    if track:
        assert torch.equal(rm2, bn.running_mean) and torch.equal(rv2, bn.running_var)
    xc3, bn3 = xc.detach().clone().requires_grad_(True), module()
    pe.batch_norm_train_cm(xc3, T, bn3, relu_in=relu_in, keep=kd).backward(dyc)
    assert torch.equal(xc3.grad, xc.grad) and torch.equal(bn3.weight.grad, bn.weight.grad) and torch.equal(bn3.bias.grad, bn.bias.grad)
    got = {'y': _bct(y.detach(), T), 'save_mean': mean, 'save_rstd': rstd, 'dx': _bct(xc.grad, T), 'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad}
    if track:
        got.update(running_mean=bn.running_mean, running_var=bn.running_var)
    assert set(want) - set(got) == (set() if track else {'running_mean', 'running_var'})
    tag = f'bn[{B}x{T} C={C} {kind}{"" if masked else " keep=None"}{"" if track else " untracked"}]'
    for k in got:
        assert got[k].shape == want[k].shape
        E.check(f'{tag} {k}', got[k].cpu(), want[k], ref[k])


# ---------------------------------------------------------------------------------------------------------------------
# 2. GroupNorm + ReLU + residual, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
GN_CASES = [(*s, False, False) for s in E.GN_SHAPES] + [
    (3, 64, 4, 2000, False, True),                   # relu=False, residual=None
    (1, 16, 1, 8000, True, False)]                   # x = 100 + 0.1 N


@pytest.mark.parametrize('B,C,G,T,offset,plain', GN_CASES)
def test_group_norm_at_training_size(B, C, G, T, offset, plain):
    from diffsinger_amd import pe
    c, want, ref = E.gn_refs(B, C, G, T, offset, plain)
    assert c['vmin'] >= E.KINK
    xc, dyc = _cm(c['x']).requires_grad_(True), _cm(c['dy'])
    rc = None if plain else _cm(c['res']).requires_grad_(True)
    gd, bd = c['gamma'].to(DEV).requires_grad_(True), c['beta'].to(DEV).requires_grad_(True)
    y = pe.group_norm_cm(xc, T, G, gd, bd, E.EPS, relu=not plain, residual=rc)
    y.backward(dyc)
    assert _zero_tail(y, xc.grad, T=T)
    got = {'y': _bct(y.detach(), T), 'dx': _bct(xc.grad, T), 'dgamma': gd.grad, 'dbeta': bd.grad}
    if not plain:
        assert torch.equal(rc.grad, dyc)                                   # the residual's gradient is dy itself
        got['dres'] = _bct(rc.grad, T)
    assert set(got) == set(want)
    # without autograd the forward is the same launch: the same bits
    with torch.no_grad():
        assert torch.equal(pe.group_norm_cm(xc.detach(), T, G, gd.detach(), bd.detach(), E.EPS, relu=not plain,
                                            residual=None if plain else rc.detach()), y.detach())
    tag = f'gn[{B}x{C}/{G}x{T}{" offset" if offset else ""}{" relu=False residual=None" if plain else ""}]'
    for k in want:
        assert got[k].shape == want[k].shape
        E.check(f'{tag} {k}', got[k].cpu(), want[k], ref[k])
    xc2 = xc.detach().clone().requires_grad_(True)
    gd2, bd2 = gd.detach().clone().requires_grad_(True), bd.detach().clone().requires_grad_(True)
    pe.group_norm_cm(xc2, T, G, gd2, bd2, E.EPS, relu=not plain, residual=None if plain else rc.detach()).backward(dyc)
    assert torch.equal(xc2.grad, xc.grad) and torch.equal(gd2.grad, gd.grad) and torch.equal(bd2.grad, bd.grad)


def test_group_norm_backward_refuses_65_channels_per_group():
    """C / G = 65 is one more than chs[][] of k_pe_gn_bwd holds: dsf_group_norm_bwd returns an error before any launch."""
    from diffsinger_amd import _lib, pe
    B, C, G, T = 1, 130, 2, 8
    lib = _lib.load()
    x = torch.randn(B, C, E.fs_ts(T), device=DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    dx = torch.full_like(x, 7.0)
    dg, db = torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
    ws = torch.full((int(lib.dsf_group_norm_bwd_workspace_floats(B, C)),), 7.0, device=DEV)
    rc = lib.dsf_group_norm_bwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                ws.data_ptr(), B, C, G, T, 1e-5, 1, None)
    with pytest.raises(Exception, match='at most 64 channels per group'):
        _lib.check(rc, 'dsf_group_norm_bwd')
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (dx, dg, db, ws))              # nothing was written: no kernel ran
    xg = x.clone().requires_grad_(True)                                       # the same through autograd: the forward has no such limit
    y = pe.group_norm_cm(xg, T, G, gamma, beta, 1e-5, relu=True)
    with pytest.raises(Exception, match='at most 64 channels per group'):
        y.backward(torch.ones_like(y))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the pitch loss, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
F0_CASES = [(B, T, 2, 'l1', True) for B, T in E.F0_SHAPES] + [(4, 17500, 2, 'l2', False), (10, 2000, 3, 'l1', True)]


@pytest.mark.parametrize('B,T,Cp,pitch_loss,use_uv', F0_CASES)
def test_f0_loss_at_training_size(B, T, Cp, pitch_loss, use_uv):
    from diffsinger_amd.pe import f0_loss_terms
    c, hp, want, ref = E.f0_refs(B, T, Cp, pitch_loss, use_uv)
    f0, uv, nonpadding = c['f0'].to(DEV), c['uv'].to(DEV), c['nonpadding'].to(DEV)

    def run():
        base = c['pred'].permute(2, 0, 1).contiguous().to(DEV).requires_grad_(True)    # [Cp,B,T]: the [B,T,Cp] view of it is not contiguous
        view = base.permute(1, 2, 0)
        assert not view.is_contiguous()
        t = f0_loss_terms(view, f0, uv, nonpadding, use_uv=use_uv, pitch_loss=pitch_loss, lam_uv=hp['lambda_uv'], lam_f0=hp['lambda_f0'])
        (E.W_UV * t[0] + E.W_F0 * t[1]).backward()
        return t.detach().cpu(), base.grad.permute(1, 2, 0).cpu()
    t, dpred = run()
    got = {'f0': t[1], 'dpred': dpred}
    if use_uv:
        got['uv'] = t[0]
    assert set(got) == set(want)
    # every frame: dpred has a value for each of them (it is written into an uninitialised tensor), exactly zero on the padding frames, in
    # the channels the loss does not read and, under use_uv, in the f0 channel of every unvoiced frame
    assert dpred.shape == want['dpred'].shape == (B, T, Cp) and bool(torch.isfinite(dpred).all())
    assert float(dpred[..., 2:].abs().sum()) == 0.0
    assert float(dpred[c['nonpadding'] == 0].abs().sum()) == 0.0
    if use_uv:
        assert float(dpred[..., 0][c['uv'] == 1].abs().sum()) == 0.0
    else:
        assert float(dpred[..., 1:].abs().sum()) == 0.0
    live = (c['nonpadding'] * (c['uv'] == 0)) > 0 if use_uv else c['nonpadding'] > 0
    assert bool((dpred[..., 0][live] != 0).all())
    assert float(t[3]) == float(live.sum())                                             # the mask sums are integers below 2^24: exact
    if use_uv:
        assert float(t[2]) == float(c['nonpadding'].sum())
    tag = f'f0_loss[{B}x{T}x{Cp} {pitch_loss} uv={use_uv}]'
    for k in want:
        E.check(f'{tag} {k}', got[k], want[k], ref[k])
    t2, dpred2 = run()
    assert torch.equal(t2, t) and torch.equal(dpred2, dpred)                            # two evaluations are bitwise equal


# ---------------------------------------------------------------------------------------------------------------------
# 4. BatchNorm in eval mode: y = (x a + b) keep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,T,keep', E.AFFINE_SHAPES)
def test_channel_affine_elementwise(B, C, T, keep):
    from diffsinger_amd.pe import channel_affine_cm
    x, a, b, k = E.affine_case(B, C, T, keep)
    want, tol = E.affine_reference(x, a, b, k)
    TS = E.fs_ts(T)
    xc = torch.full((B, C, TS), 3.0)                                       # the tail of the input is not zero: the kernel must not pass it on
    xc[:, :, :T] = x
    got = channel_affine_cm(xc.to(DEV), T, a.to(DEV), b.to(DEV), k.to(DEV).contiguous() if k is not None else None).cpu()
    assert got.shape == (B, C, TS) and float(got[:, :, T:].abs().sum()) == 0.0
    excess = ((got[:, :, :T].double() - want).abs() - tol).max()
    share = float(((got[:, :, :T].double() - want).abs() / tol.clamp_min(1e-300)).max())
    print(f'affine[{B}x{C}x{T} keep={keep}]: {B * C * TS // 4} float4s, largest share of the per-element bound {share:.2f}')
    assert float(excess) <= 0.0
    if k is not None:
        assert float(got[:, :, :T][k[:, None, :].expand(B, C, T) == 0].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the module in eval mode at a long length
# ---------------------------------------------------------------------------------------------------------------------
def test_pitch_extractor_eval_at_1100_frames():
    from oracle import pe_oracle as PO
    g, hp, p, m = _build(77)
    B, T = 2, 1100
    mel = PO.synth_mel(B, T, 9)
    mel[1, T - 300:] = 0                                                   # one utterance ends in 300 padding frames
    with torch.no_grad():
        want = PO.pitch_extractor(p, hp, mel)
    r = m(mel.to(DEV))
    assert r['pitch_pred'].shape == (B, T, 2)
    _compare(r, want['pitch_pred'].numpy(), want['f0_denorm_pred'].numpy())
    assert bool((r['f0_denorm_pred'].cpu()[1, T - 300:] == 0).all())
