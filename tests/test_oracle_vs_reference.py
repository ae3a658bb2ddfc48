"""The oracle restatement against what the LIVE reference computed on a configuration the goldens do not cover (narrow model, dilation
cycle 2, cosine schedule, per-step comparison of p_sample / q_sample / p_sample_plms; p_losses and the gradients of all parameters, with and
without the non-padding mask - the oracle of the training row).  The reference's side is recorded in tests/golden/live_diffnet_<sched>.npz
by oracle/make_golden_live.py (build container); parameters and gradients as sha256 digests, everything else as arrays - bit for bit."""
import os
from collections import deque

import numpy as np
import pytest
import torch

from oracle import diffnet_oracle as O
from oracle.make_golden_live import diffnet_inputs, digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eq(a, want, what):
    assert np.array_equal(a.detach().numpy(), want), (what, float(np.abs(a.detach().numpy() - want).max()))


@pytest.mark.parametrize('sched', ['linear', 'cosine'])
def test_oracle_bit_equal_to_live_reference(sched):
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', f'live_diffnet_{sched}.npz'))
    cfg = O.NetConfig(20, 32, 48, 5, 2)
    p = O.init_diffnet_params(cfg, 7, 0.05)
    assert list(p) == list(ref['param_keys'])
    for k, d in zip(ref['param_keys'], ref['param_digests']):
        assert digest(p[k]) == d, k
    betas = O.linear_beta_schedule(50, 0.06) if sched == 'linear' else O.cosine_beta_schedule(50)
    sch = O.make_schedule(betas)
    for k, v in sch.items():
        _eq(v, ref[f'sch_{k}'], k)
    inp = diffnet_inputs(torch)
    for k, v in inp.items():
        _eq(v, ref[f'in_{k}'], k)
    x, cond, z, mel = inp['x'], inp['cond'], inp['z'], inp['mel']
    with torch.no_grad():
        t = torch.tensor([49, 7, 0])
        _eq(O.diffnet_forward(p, cfg, x, t, cond), ref['eps'], 'forward')
        _eq(O.p_sample(p, cfg, sch, x, t, cond, z), ref['p_sample'], 'p_sample')
        _eq(O.q_sample(sch, x, torch.tensor([30]), z), ref['q_sample'], 'q_sample')
        sm, sx = torch.from_numpy(ref['spec_min']), torch.from_numpy(ref['spec_max'])
        _eq(O.norm_spec(mel, sm, sx), ref['norm_spec'], 'norm_spec')
        _eq(O.denorm_spec(mel, sm, sx), ref['denorm_spec'], 'denorm_spec')
        # PLMS, B = 1 (the only batch size the reference supports), every warm-up order + t < interval tail
        xo, cb, hist = x[:1], cond[:1], deque(maxlen=4)
        for i in reversed(range(0, 50, 8)):
            xo = O.p_sample_plms(p, cfg, sch, xo, torch.full((1,), i, dtype=torch.long), 8, cb, hist)
            _eq(xo, ref[f'plms_{i}'], f'plms {i}')
    # training (row f3): p_losses and the gradient of EVERY parameter - torch autograd on the oracle vs the reference module under autograd
    for tag, nonpad in (('nomask', None), ('mask', inp['nonpad'])):
        tt = torch.tensor([49, 7, 0])
        po = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        diff = z - O.diffnet_forward(po, cfg, O.q_sample(sch, x, tt, z), tt, cond)
        loss_o = (diff.abs() * nonpad.unsqueeze(1)).mean() if nonpad is not None else diff.abs().mean()
        loss_o.backward()
        _eq(loss_o, ref[f'loss_{tag}'], f'loss {tag}')
        for k, d in zip(ref[f'grad_{tag}_keys'], ref[f'grad_{tag}_digests']):
            assert po[k].grad is not None, k
            assert digest(po[k].grad) == d, (tag, k)
