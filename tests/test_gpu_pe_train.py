"""GPU: the PitchExtractor TRAINING path on HIP (PitchExtractionTask, tasks/tts/pe.py) - the BatchNorm training operator, the GroupNorm backward
and the fused pitch loss against float64 torch, the module against the fixture recorded from the reference's own PitchExtractor().train()
(tests/golden/pe_train_ref.npz) and, at the real width, against the float64 restatement of tests/pe_train_helpers.py.

Tolerance rule (pe_train_helpers.bound): for a tensor X the error is max|X_hip - X_64| / max|X_64|; it may be at most 4 x the error of the fp32
CPU reference on the same tensor (F.batch_norm / F.group_norm / autograd on the CPU, or the deviation stored in the fixture), floor 2e-6.  No
element is ever excluded: the cases are chosen so that no ReLU input is near its kink (asserted)."""
import ast
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffsinger_amd import hparams
from oracle import pe_oracle as PO
from tests import pe_edge_helpers as E
from tests import pe_train_helpers as PH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDE = dict(PH.HP, hidden_size=256)                 # the shipped width: GroupNorm(16, 256), LayerNorm over 256 channels
WIDE_CASE = dict(B=2, T=40, seed=506)           # the first seed from 501 that meets the 8x ReLU condition on the CPU


_check = E.check                                    # shared with tests/test_gpu_pe_edges.py


def _check_dev(name, got, x64, dev):
    err = PH.rel_err(got, x64)
    print(f'{name}: err {err:.3e}  fp32 reference {dev:.3e}  bound {PH.bound(dev):.3e}')
    assert err <= PH.bound(dev), (name, err, dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. BatchNorm on batch statistics
# ---------------------------------------------------------------------------------------------------------------------
_bn_reference = E.bn_reference                      # y = native_batch_norm(relu(x)) * keep and its gradients under L = sum(y dy)


@pytest.mark.parametrize('B,T,kind', [(3, 75, 'kink_free'), (1, 2, 'kink_free'), (3, 75, 'cancellation')])
def test_batch_norm_train_operator(B, T, kind):
    from diffsinger_amd import pe
    from diffsinger_amd.fs2 import from_cm, to_cm
    C = 64
    g = torch.Generator().manual_seed(11 + B)
    if kind == 'cancellation':                       # mean 100, spread 0.1: E[x^2] - E[x]^2 would lose every digit of the variance
        x, relu_in = 100 + 0.1 * torch.randn(B, C, T, generator=g), False
    else:                                            # no ReLU input near zero
        x, relu_in = torch.randn(B, C, T, generator=g), True
        x = torch.sign(x) * (x.abs() + 0.01)
    keep = torch.ones(B, T)
    for b in range(B):
        keep[b, T - 1 - 7 * b:] = 0                  # ragged (B = 1: the last frame)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    dy = torch.randn(B, C, T, generator=g)
    want, ref = (_bn_reference(x, gamma, beta, rm, rv, keep, dy, relu_in, dt) for dt in (torch.float64, torch.float32))

    bn = torch.nn.BatchNorm1d(C).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    kd = keep.to(DEV).contiguous()
    xc = to_cm(x.transpose(1, 2).to(DEV)).requires_grad_(True)
    y = pe.batch_norm_train_cm(xc, T, bn, relu_in=relu_in, keep=kd)
    y.backward(to_cm(dy.transpose(1, 2).to(DEV)))
    assert int(bn.num_batches_tracked) == 1
    assert float(y.detach()[:, :, T:].abs().sum()) == 0.0 and float(xc.grad[:, :, T:].abs().sum()) == 0.0
    # the statistics, and a second run: bit for bit the same
    rm2, rv2 = rm.to(DEV), rv.to(DEV)
    y2, mean, rstd = pe._batch_norm_train_raw(xc.detach(), T, bn.weight.detach(), bn.bias.detach(), rm2, rv2, bn.eps, bn.momentum, relu_in, kd)
    assert torch.equal(y2, y.detach()) and torch.equal(rm2, bn.running_mean) and torch.equal(rv2, bn.running_var)
    xc3 = xc.detach().clone().requires_grad_(True)
    bn3 = torch.nn.BatchNorm1d(C).to(DEV).train()
    bn3.load_state_dict({**bn.state_dict(), 'running_mean': rm.to(DEV), 'running_var': rv.to(DEV)})
    pe.batch_norm_train_cm(xc3, T, bn3, relu_in=relu_in, keep=kd).backward(to_cm(dy.transpose(1, 2).to(DEV)))
    assert torch.equal(xc3.grad, xc.grad) and torch.equal(bn3.weight.grad, bn.weight.grad) and torch.equal(bn3.bias.grad, bn.bias.grad)
    got = {'y': from_cm(y.detach(), T).transpose(1, 2), 'save_mean': mean, 'save_rstd': rstd, 'running_mean': bn.running_mean,
           'running_var': bn.running_var, 'dx': from_cm(xc.grad, T).transpose(1, 2), 'dgamma': bn.weight.grad, 'dbeta': bn.bias.grad}
    for k in want:
        _check(f'bn[{B}x{T} {kind}] {k}', got[k].cpu(), want[k], ref[k])


# ---------------------------------------------------------------------------------------------------------------------
# 2. GroupNorm + ReLU + residual, backward
# ---------------------------------------------------------------------------------------------------------------------
def _gn_case(B, C, G, T):
    """Seeded inputs whose float64 pre-ReLU values keep min|v| >= 1e-4 (the first seed that does)."""
    for seed in range(100, 200):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, C, T, generator=g) * 2 + 0.5
        gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        res, dy = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
        v = F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-5)
        if float(v.abs().min()) >= 1e-4:
            return x, gamma, beta, res, dy, float(v.abs().min())
    raise AssertionError('no seed keeps the pre-ReLU values away from zero')


_gn_reference = E.gn_reference                      # y = res + relu(group_norm(x)) and its gradients under L = sum(y dy)


@pytest.mark.parametrize('B,C,G,T', [(3, 64, 4, 75), (2, 256, 16, 40)])
def test_group_norm_backward_operator(B, C, G, T):
    from diffsinger_amd import pe
    from diffsinger_amd.fs2 import from_cm, to_cm
    x, gamma, beta, res, dy, vmin = _gn_case(B, C, G, T)
    assert vmin >= 1e-4
    want, ref = (_gn_reference(x, gamma, beta, res, dy, G, dt) for dt in (torch.float64, torch.float32))
    xc = to_cm(x.transpose(1, 2).to(DEV)).requires_grad_(True)
    rc = to_cm(res.transpose(1, 2).to(DEV)).requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    dyc = to_cm(dy.transpose(1, 2).to(DEV))
    y = pe.group_norm_cm(xc, T, G, gd, bd, 1e-5, relu=True, residual=rc)
    y.backward(dyc)
    assert torch.equal(rc.grad, dyc)                                   # the residual's gradient is dy itself
    assert float(y.detach()[:, :, T:].abs().sum()) == 0.0 and float(xc.grad[:, :, T:].abs().sum()) == 0.0
    got = {'y': from_cm(y.detach(), T).transpose(1, 2), 'dx': from_cm(xc.grad, T).transpose(1, 2), 'dgamma': gd.grad, 'dbeta': bd.grad,
           'dres': from_cm(rc.grad, T).transpose(1, 2)}
    for k in want:
        _check(f'gn[{B}x{C}/{G}x{T}] {k}', got[k].cpu(), want[k], ref[k])
    xc2 = xc.detach().clone().requires_grad_(True)
    gd2, bd2 = gd.detach().clone().requires_grad_(True), bd.detach().clone().requires_grad_(True)
    pe.group_norm_cm(xc2, T, G, gd2, bd2, 1e-5, relu=True, residual=rc.detach()).backward(dyc)
    assert torch.equal(xc2.grad, xc.grad) and torch.equal(gd2.grad, gd.grad) and torch.equal(bd2.grad, bd.grad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the pitch loss
# ---------------------------------------------------------------------------------------------------------------------
def _loss_reference(pred, f0, uv, nonpadding, hp, dtype):
    p = pred.to(dtype).clone().requires_grad_(True)
    losses = PH.f0_losses(p, f0.to(dtype), uv.to(dtype), nonpadding.to(dtype), hp)
    (1.3 * losses.get('uv', 0) + 0.7 * losses['f0']).backward()
    return {**{k: v.detach() for k, v in losses.items()}, 'dpred': p.grad}


@pytest.mark.parametrize('pitch_loss', ['l1', 'l2'])
@pytest.mark.parametrize('use_uv', [True, False])
def test_f0_loss_operator(pitch_loss, use_uv):
    from diffsinger_amd.pe import f0_loss_terms, pe_losses
    B, T = 3, 301                                            # more than one 256-thread block of frames
    g = torch.Generator().manual_seed(5)
    hp = dict(PH.HP, pitch_loss=pitch_loss, use_uv=use_uv, lambda_f0=0.7 if pitch_loss == 'l2' else 1.0, lambda_uv=1.5)
    pred = torch.stack([7.5 + 0.5 * torch.randn(B, T, generator=g), 2 * torch.randn(B, T, generator=g)], -1)
    pred[0, 3, 1], pred[1, 4, 1], pred[2, 5, 1], pred[2, 6, 1] = 40.0, -40.0, 40.0, -40.0        # the overflow-safe BCE form
    f0, uv = 7.5 + 0.5 * torch.randn(B, T, generator=g), (torch.rand(B, T, generator=g) < 0.3).float()
    uv[1] = 1.0                                              # one row entirely unvoiced
    uv[0, 3], uv[1, 4], uv[2, 5], uv[2, 6] = 1.0, 1.0, 0.0, 0.0
    nonpadding = torch.ones(B, T)
    nonpadding[1, T - 40:], nonpadding[2, T - 90:] = 0, 0
    want, ref = (_loss_reference(pred, f0, uv, nonpadding, hp, dt) for dt in (torch.float64, torch.float32))
    base = pred.permute(2, 0, 1).contiguous().to(DEV).requires_grad_(True)     # [2,B,T]: the [B,T,2] view of it is not contiguous
    view = base.permute(1, 2, 0)
    assert not view.is_contiguous()
    t = f0_loss_terms(view, f0.to(DEV), uv.to(DEV), nonpadding.to(DEV), use_uv=use_uv, pitch_loss=pitch_loss, lam_uv=hp['lambda_uv'], lam_f0=hp['lambda_f0'])
    (1.3 * t[0] + 0.7 * t[1]).backward()
    got = {'f0': t[1].detach().cpu(), 'dpred': base.grad.permute(1, 2, 0).cpu()}
    if use_uv:
        got['uv'] = t[0].detach().cpu()
    assert set(got) == set(want)
    for k in want:
        _check(f'f0_loss[{pitch_loss} uv={use_uv}] {k}', got[k], want[k], ref[k])
    mel = nonpadding[:, :, None].expand(B, T, 80).to(DEV)
    d = pe_losses({'pitch_pred': view.detach()}, {'mels': mel, 'f0': f0.to(DEV), 'uv': uv.to(DEV)}, hp)
    assert list(d) == (['uv', 'f0'] if use_uv else ['f0'])
    assert all(torch.equal(d[k].cpu(), got[k]) for k in d)   # two evaluations are bitwise equal


# ---------------------------------------------------------------------------------------------------------------------
# 4-7. the module
# ---------------------------------------------------------------------------------------------------------------------
def _module(hp, state, dropout=0.0):
    hparams.clear()
    hparams.update(hp, dur_loss='mse')
    from diffsinger_amd.pe import PitchExtractor
    m = PitchExtractor().train()
    m.load_state_dict(state, strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = dropout
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _wide_reference():
    state, mel, f0, uv = PH.case_inputs(WIDE, **WIDE_CASE)
    return state, mel, f0, uv, PH.training_step(state, WIDE, mel, f0, uv, torch.float64), PH.training_step(state, WIDE, mel, f0, uv, torch.float32)


def _compare_step(m, losses, total, pitch_pred, want, dev_of):
    total.backward()
    _check_dev('pitch_pred', pitch_pred.detach().cpu(), want['pitch_pred'], dev_of('pitch_pred'))
    for k in ('uv', 'f0'):
        _check_dev('loss/' + k, losses[k].detach().cpu(), want[k], dev_of('loss/' + k))
    params = dict(m.named_parameters())
    assert set(params) == set(want['grad'])
    for k, v in params.items():
        _check_dev('grad/' + k, v.grad.cpu(), want['grad'][k], dev_of('grad/' + k))
    sd = m.state_dict()
    for k, v in want['running'].items():
        if k.endswith('num_batches_tracked'):
            assert int(sd[k]) == int(v) == 8
        else:
            _check_dev('running/' + k, sd[k].cpu(), v, dev_of('running/' + k))


def test_module_matches_reference_fixture():
    g = np.load(PH.FIXTURE)
    hp = ast.literal_eval(str(g['hp']))
    state, mel, f0, uv = PH.case_inputs(hp, int(g['B']), int(g['T']), int(g['seed']))
    want = PH.training_step(state, hp, mel, f0, uv, torch.float64)
    m = _module(hp, state)
    from diffsinger_amd.pe import pe_training_step
    seen = {}
    m.register_forward_hook(lambda _m, _inp, out: seen.update(out))            # the step's own forward: a second one would update the buffers again
    total, losses = pe_training_step(m, {'mels': mel.to(DEV), 'f0': f0.to(DEV), 'uv': uv.to(DEV)}, hp)
    assert list(losses) == ['uv', 'f0', 'batch_size'] and losses['batch_size'] == int(g['B'])
    pitch_pred = seen['pitch_pred']
    _compare_step(m, losses, total, pitch_pred, want, lambda k: float(g['dev/' + k]))
    # the recorded fp32 reference itself, within both errors
    assert PH.rel_err(pitch_pred.detach().cpu(), torch.from_numpy(g['pitch_pred'])) <= PH.bound(float(g['dev/pitch_pred'])) + float(g['dev/pitch_pred'])
    assert any('libdsdenoise' in ln for ln in open('/proc/self/maps'))


def test_module_at_the_real_width():
    state, mel, f0, uv, want, ref = _wide_reference()
    ratio, flips = PH.relu_condition(ref['relu'], want['relu'])
    print('smallest ReLU ratio', ratio, 'sign disagreements', flips)
    assert flips == 0 and ratio >= PH.RELU_MARGIN
    dev = {'pitch_pred': PH.rel_err(ref['pitch_pred'], want['pitch_pred']), 'loss/uv': PH.rel_err(ref['uv'], want['uv']),
           'loss/f0': PH.rel_err(ref['f0'], want['f0'])}
    dev.update({'grad/' + k: PH.rel_err(v, want['grad'][k]) for k, v in ref['grad'].items()})
    dev.update({'running/' + k: PH.rel_err(v, want['running'][k]) for k, v in ref['running'].items() if not k.endswith('num_batches_tracked')})
    m = _module(WIDE, state)
    from diffsinger_amd.pe import pe_losses
    sample = {'mels': mel.to(DEV), 'f0': f0.to(DEV), 'uv': uv.to(DEV)}
    out = m(sample['mels'])
    losses = pe_losses(out, sample, WIDE)
    total = losses['uv'] + losses['f0']
    assert out['f0_denorm_pred'].shape == (WIDE_CASE['B'], WIDE_CASE['T'])
    _compare_step(m, losses, total, out['pitch_pred'], want, lambda k: dev[k])


def test_eval_after_train_uses_the_updated_statistics():
    state, mel, f0, uv = PH.case_inputs()
    m = _module(PH.HP, state)
    before = {k: v.clone() for k, v in m.state_dict().items() if 'running' in k}
    m(mel.to(DEV))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert all(not torch.equal(sd[k], before[k].cpu()) for k in before)
    r = m.eval()(mel.to(DEV))
    assert not r['pitch_pred'].requires_grad
    with torch.no_grad():
        want = PO.pitch_extractor(sd, PH.HP, mel)
    err = float((r['pitch_pred'].cpu() - want['pitch_pred']).abs().max())
    print('eval after train: pitch_pred err', err)
    assert err < 2e-4, err


def test_twenty_adamw_steps_reduce_the_loss():
    from diffsinger_amd.pe import pe_training_step
    torch.manual_seed(7)
    state, mel, f0, uv = PH.case_inputs()
    m = _module(PH.HP, state, dropout=0.1)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    sample = {'mels': mel.to(DEV), 'f0': f0.to(DEV), 'uv': uv.to(DEV)}
    hist = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        total, losses = pe_training_step(m, sample, PH.HP)
        total.backward()
        opt.step()
        hist.append(total.detach())
    hist = torch.stack(hist).cpu()
    print('losses', [round(float(v), 4) for v in hist])
    assert bool(torch.isfinite(hist).all())
    assert float(hist[-1]) < float(hist[0])
    assert int(m.mel_prenet.layers[0][2].num_batches_tracked) == 7 + 20
