"""Shared by tests/test_voc_optim_host.py, tests/test_gpu_voc_optim.py and tools/make_golden_voc_optim.py: the inputs' recipe, a restatement of the
two optimisers that runs in any float type (float64: the truth; float32 on the CPU: the stand-in for a reference run where the fixture has
none), and the ONE error bound every comparison uses.

The bound, per tensor after S steps:      max|x - x64| <= 4 * max|x_ref32 - x64| + S * 2^-23 * max|x64|
x is p, exp_avg or exp_avg_sq; x_ref32 the fixture (the reference's RAdam, float32, CPU) or the restatement in float32.  The floor is one rounding
of the value per step, doubled for two orders of evaluation.

The inputs are built so that an error would show: lr = 0.1 on parameters of magnitude 0.01, eps = 1e-6, and per-tensor gradient scales 1e-5, 1e-3,
1 and 30 - at 1e-5 sqrt(v) is about 8e-7, the order of eps, so where eps is added shows."""
import math
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'voc_optim_ref.npz')
FIXTURE_SIZES = (1, 3, 5, 64, 1027)
# The host test holds the REFERENCE'S OWN float32 run to the floor alone (no 4 x term), and that is not a property of every draw: at step 1,
# exp_avg_sq = ((1 - b2) g) g carries the conversion of 1 - 0.999 to float32 (0.4 of the floor by itself) and two product roundings, 1.4 of the
# floor at worst on the largest element.  Over the seeds 20240..20251 the reference's worst error / floor was 1.14 0.89 0.87 1.01 0.75 0.73 0.89
# 1.74 1.99 1.13 0.76 0.80; the fixture is recorded at one where the reference stays inside (0.73).  No figure of the HIP kernels entered the choice.
FIXTURE_SEED = 20245
STEPS = 8
GRAD_SCALES = (1e-5, 1e-3, 1.0, 30.0)
SETTINGS = {'b999': dict(lr=0.1, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0),
            'b99wd': dict(lr=0.1, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)}
ULP = 2.0 ** -23


def inputs(sizes, seed, steps=STEPS):
    """-> (p0: one float32 tensor per size, magnitude 0.01; grads[step][tensor] float32, tensor i at scale GRAD_SCALES[i % 4]).  A gradient is a
    direction that persists over the steps (magnitude in [0.5, 1.5), random sign) plus half a unit of noise per step, as the gradients of a
    training run are: every tensor then moves steadily, a one-element tensor included, and the guard of check_not_empty holds for every seed
    instead of by the luck of one draw."""
    rs = np.random.RandomState(seed)
    p0 = [torch.from_numpy((0.01 * rs.standard_normal(n)).astype(np.float32)) for n in sizes]
    drift = [rs.choice([-1.0, 1.0], n) * (0.5 + rs.random_sample(n)) for n in sizes]
    grads = [[torch.from_numpy((GRAD_SCALES[i % 4] * (drift[i] + 0.5 * rs.standard_normal(n))).astype(np.float32)) for i, n in enumerate(sizes)]
             for _ in range(steps)]
    return p0, grads


def radam_scalars(step, beta1, beta2):
    """N_sma, step_size, rectified - the scalars of the reference's step in Python floats"""
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** step)
    else:
        size = 1.0 / (1 - beta1 ** step)
    return n_sma, size, n_sma >= 5


def radam_update(p, g, m, v, step, lr, betas, eps, weight_decay):
    """one RAdam step on tensors of one float type, in place"""
    b1, b2 = betas
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    m.mul_(b1).add_(g, alpha=1 - b1)
    _, size, rect = radam_scalars(step, b1, b2)
    if weight_decay != 0:
        p.add_(p, alpha=-weight_decay * lr)
    if rect:
        p.addcdiv_(m, v.sqrt().add_(eps), value=-size * lr)
    else:
        p.add_(m, alpha=-size * lr)


def adamw_update(p, g, m, v, step, lr, betas, eps, weight_decay):
    """one torch.optim.AdamW step (amsgrad off) on tensors of one float type, in place"""
    b1, b2 = betas
    p.mul_(1 - lr * weight_decay)
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(eps), value=-(lr / bc1))


def restate(update, p0, grads, hp, dtype, gscale=None, first_step=1):
    """The trajectory of `update` in `dtype` on the CPU -> per step (p, m, v), each a list of tensors.  grads[s][i] None: tensor i is skipped at that
    step and its own step count does not advance.  gscale: every gradient is multiplied by it first (in `dtype`)."""
    p = [t.to(dtype).clone() for t in p0]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    count = [first_step - 1] * len(p)
    out = []
    for gs in grads:
        for i, g in enumerate(gs):
            if g is None:
                continue
            g = g.to(dtype)
            if gscale is not None:
                g = g * torch.tensor(gscale, dtype=dtype)
            count[i] += 1
            update(p[i], g, m[i], v[i], count[i], **hp)
        out.append(([t.clone() for t in p], [t.clone() for t in m], [t.clone() for t in v]))
    return out


def bound(x64, ref32, steps):
    return 4.0 * float((ref32.double() - x64).abs().max()) + steps * ULP * float(x64.abs().max())


def floor(x64, steps):
    return steps * ULP * float(x64.abs().max())


def check_trajectory(name, got, t64, t32):
    """got, t64, t32: per step (p, m, v) lists; asserts the bound for every tensor at every step -> the largest error / bound ratio seen"""
    worst = 0.0
    for s, (gs, ws, rs) in enumerate(zip(got, t64, t32)):
        for kind, ga, wa, ra in zip(('p', 'exp_avg', 'exp_avg_sq'), gs, ws, rs):
            for i, (x, x64, x32) in enumerate(zip(ga, wa, ra)):
                err, b = float((x.double().cpu() - x64).abs().max()), bound(x64, x32, s + 1)
                assert err <= b, (name, kind, 'step', s + 1, 'tensor', i, err, b)
                worst = max(worst, err / b if b > 0 else 0.0)             # b = 0: a tensor that is all zero (the moments of a skipped one), err = 0
    return worst


def check_not_empty(name, p0, t64, t32):
    """the guard against an empty test: steps 1-5 (the unrectified branch) and steps 6-8 (the rectified one) each move every tensor by at least
    100 x the bound it is checked with"""
    for first, last in ((0, 5), (5, 8)):
        for i in range(len(p0)):
            before = p0[i].double() if first == 0 else t64[first - 1][0][i]
            moved = float((t64[last - 1][0][i] - before).abs().max())
            b = bound(t64[last - 1][0][i], t32[last - 1][0][i], last)
            assert moved >= 100 * b, (name, 'steps', first + 1, last, 'tensor', i, moved, b)


def load_fixture():
    """-> (p0, grads, {setting: per step (p, m, v)}) as float32 CPU tensors"""
    z = np.load(FIXTURE)
    n = len(FIXTURE_SIZES)
    p0 = [torch.from_numpy(z[f'p0/{i}']) for i in range(n)]
    grads = [[torch.from_numpy(z[f'g/{s}/{i}']) for i in range(n)] for s in range(STEPS)]
    traj = {k: [tuple([torch.from_numpy(z[f'{k}/{x}/{s}/{i}']) for i in range(n)] for x in ('p', 'm', 'v')) for s in range(STEPS)] for k in SETTINGS}
    return p0, grads, traj
