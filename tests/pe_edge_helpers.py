"""Test infrastructure of the PitchExtractor edge tests (tests/test_pe_edges_host.py, tests/test_gpu_pe_edges.py): the norms of the training
path and the pitch loss at the sizes a training step has.  CPU only: nothing here touches the HIP library.

Yardsticks.  The float64 yardstick is the one of tests/test_gpu_pe_train.py (torch.native_batch_norm, F.group_norm, pe_train_helpers.f0_losses
under autograd).  The float32 yardstick, whose own error sets the bound (pe_train_helpers.bound: 4 x, floor 2e-6), is NOT aten's float32 kernel
at these lengths: aten's CPU BatchNorm / GroupNorm accumulate the float statistics in double and keep the mean in double, so their float32
error is far below that of any float32 summation (4.5e-7 against 5.0e-6 for a correct fixed-order float32 kernel on x = 100 + 0.1 N(0,1) at
3 x 8000).  Each operator therefore has an elementary restatement from plain torch ops in which every intermediate is a tensor of the working
dtype (bn_restated, gn_restated, f0_restated):

    mean = r.sum() / n ; e = r - mean ; var = (e * e).sum() / n ; rstd = 1 / sqrt(var + eps) ; y = e * rstd * gamma + beta ; then the mask

with the gradients by autograd through it.  In float32 it is the yardstick; in float64 it equals the float64 yardstick to 1e-12 and on small
shapes in float32 aten's result to a few ulp (the host test).

Kinks.  No element is ever left out of a comparison, so no ReLU input may sit near zero.  BatchNorm: x = sign(x) (|x| + 0.01) in front of
relu_in.  GroupNorm: a repair loop - where the float64 pre-ReLU value v has |v| < 1e-3, x moves by 0.05 sign(v) sign(gamma), at most 20 rounds.

Restated bugs.  `bug=` of the restatements evaluates a wrong formula; the host test shows that each exceeds the bound of every case where it
can be seen by 100 x or more.  To that end the frames a bug would lose carry weight: the last 32 frames of the last row of a BatchNorm case
are outliers, the pitch-loss frames from flat index 65 536 on have a larger f0 error."""
import functools
import os
import re

import torch
import torch.nn.functional as F

from tests import pe_train_helpers as PH

U = 2.0 ** -24                                   # unit roundoff of float32
EPS, MOMENTUM = 1e-5, 0.1
KINK = 1e-3                                      # smallest |pre-ReLU value| of a GroupNorm case
# the kernels' constants, restated; the host test reads them back from the sources
BN_STAGE4 = 2048                                 # kPeBnStage4 (csrc/pe_train.hpp): float4s of a channel k_pe_bn_train keeps in LDS
GN_MAX_CG = 64                                   # kPeGnMaxCg: channels per group of k_pe_gn_bwd's chs[][]
F0_FWD_FRAMES = 256 * 256                        # kPeF0Blocks blocks of 256 frames: above it k_pe_f0_partial strides its grid
F0_BWD_FRAMES = 1024 * 256                       # the 1024-block cap of k_pe_f0_bwd's grid in dsf_f0_loss_bwd
EW_BLOCKS = 16384                                # the cap of ew_grid (csrc/fs2_abi.hpp): 16 384 blocks of 256 float4s per pass of k_fs_affine

# B, T
BN_SHAPES = [(8, 1024), (8, 1025), (1, 8192), (1, 8193), (10, 2000), (2, 8000)]
BN_KINDS = ['kink_free', 'cancellation']
BN_SMALL = [(3, 75), (1, 2)]                     # the shapes of test_batch_norm_train_operator
# B, C, G, T
GN_SHAPES = [(3, 64, 4, 2000), (2, 256, 16, 1000), (1, 16, 1, 8000), (2, 64, 64, 257), (2, 48, 16, 64), (2, 128, 2, 96), (2, 32, 2, 1)]
GN_SMALL = [(3, 64, 4, 75), (2, 256, 16, 40)]    # the shapes of test_group_norm_backward_operator
# B, T
F0_SHAPES = [(10, 2000), (4, 17500), (4, 70000)]
# B, C, T, keep
AFFINE_SHAPES = [(3, 256, 75, None), (2, 8, 64, 'ragged'), (8, 256, 8193, 'ragged')]


def fs_ts(T):
    """fs_ts of csrc/fs2_abi.hpp: the padded frame count of a channel-major tensor."""
    return (T + 31) // 32 * 32


def bn_staged(B, T):
    return B * fs_ts(T) // 4 <= BN_STAGE4


def kernel_constants():
    """The constants above as the sources state them."""
    src = os.path.join(PH.ROOT, 'diffsinger_amd', 'csrc')
    pe, abi = open(os.path.join(src, 'pe_train.hpp')).read(), open(os.path.join(src, 'fs2_abi.hpp')).read()
    num = lambda pat, text: int(re.search(pat, text).group(1))
    return {'BN_STAGE4': num(r'constexpr int kPeBnStage4 = (\d+);', pe), 'GN_MAX_CG': num(r'constexpr int kPeGnMaxCg = (\d+);', pe),
            'F0_FWD_FRAMES': num(r'constexpr int kPeF0Blocks = (\d+);', pe) * 256,
            'F0_BWD_FRAMES': num(r'k_pe_f0_bwd, dim3\(\(unsigned\)std::min<long long>\((\d+),', pe) * 256,
            'EW_BLOCKS': num(r'ew_grid\(size_t n4\) \{ return dim3\(\(unsigned\)std::min<size_t>\(\(n4 \+ 255\) / 256, (\d+)\)', abi)}


def check(name, got, x64, ref32):
    """The comparison of tests/test_gpu_pe_train.py: rel_err of `got` at most pe_train_helpers.bound of the fp32 yardstick's.  Returns the share
    of the bound that was used."""
    err, ref = PH.rel_err(got, x64), PH.rel_err(ref32, x64)
    print(f'{name}: err {err:.3e}  fp32 reference {ref:.3e}  bound {PH.bound(ref):.3e}  share {err / PH.bound(ref):.2f}')
    assert err <= PH.bound(ref), (name, err, ref)
    return err / PH.bound(ref)


def worst_ratio(got, want, ref):
    """max over the tensors of (error of got) / (bound of that tensor): what a wrong formula reaches against the bound of its case."""
    return max(PH.rel_err(got[k], want[k]) / PH.bound(PH.rel_err(ref[k], want[k])) for k in want if k in got)


# ----------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm on batch statistics
# ----------------------------------------------------------------------------------------------------------------------------------------
def bn_reference(x, gamma, beta, rm, rv, keep, dy, relu_in, dtype):
    """y = native_batch_norm(relu(x)) * keep and its gradients under L = sum(y dy), on [B,C,T] tensors in `dtype` (aten)."""
    x = x.to(dtype).clone().requires_grad_(True)
    gamma, beta = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    r = F.relu(x) if relu_in else x
    y, mean, rstd = torch.native_batch_norm(r, gamma, beta, rm, rv, True, MOMENTUM, EPS)
    y = y * keep.to(dtype)[:, None, :]
    (y * dy.to(dtype)).sum().backward()
    return {'y': y.detach(), 'save_mean': mean.detach(), 'save_rstd': rstd.detach(), 'running_mean': rm, 'running_var': rv, 'dx': x.grad,
            'dgamma': gamma.grad, 'dbeta': beta.grad}


def bn_restated(x, gamma, beta, rm, rv, keep, dy, relu_in, dtype, bug=None):
    """The same from elementary ops in `dtype`.  bug: 'first8192' (statistics over the first 8192 values of a channel's [B][TS] rows, what an
    overflow of the LDS stage would leave), 'ts_cols' (statistics over TS columns, the zero tail counted), 'biased' (running_var from the biased
    variance), 'e2' (var = E[x^2] - E[x]^2)."""
    x = x.to(dtype).clone().requires_grad_(True)
    gamma, beta = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    r = F.relu(x) if relu_in else x
    B, C, T = r.shape
    TS = fs_ts(T)
    n = B * T
    if bug == 'first8192':
        w = ((torch.arange(B * TS).view(B, TS) < 4 * BN_STAGE4)[:, :T]).to(dtype)[:, None, :]
        n = float(w.sum())
        mean = (r * w).sum((0, 2)) / n
        e = r - mean[None, :, None]
        var = (e * e * w).sum((0, 2)) / n
    elif bug == 'ts_cols':
        n = B * TS
        mean = r.sum((0, 2)) / n
        e = r - mean[None, :, None]
        var = ((e * e).sum((0, 2)) + (B * (TS - T)) * mean * mean) / n
    else:
        mean = r.sum((0, 2)) / n
        e = r - mean[None, :, None]
        var = (e * e).sum((0, 2)) / n
        if bug == 'e2':
            var = ((r * r).sum((0, 2)) / n - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + EPS)
    y = e * rstd[None, :, None] * gamma[None, :, None] + beta[None, :, None]
    y = y * keep.to(dtype)[:, None, :]
    (y * dy.to(dtype)).sum().backward()
    out = {'y': y.detach(), 'save_mean': mean.detach(), 'save_rstd': rstd.detach(), 'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad}
    unbiased = var.detach() if bug == 'biased' else var.detach() * n / (n - 1)
    out['running_mean'] = (1 - MOMENTUM) * rm.to(dtype) + MOMENTUM * mean.detach()
    out['running_var'] = (1 - MOMENTUM) * rv.to(dtype) + MOMENTUM * unbiased
    return out


@functools.lru_cache(maxsize=None)
def bn_case(B, T, kind, C=8):
    """Seeded inputs [B,C,T] of a BatchNorm case: the recipe of test_batch_norm_train_operator, a keep mask that is ragged per row, and the
    last 32 frames of the last row as outliers (4 x the value; +1 on the cancellation input, ten standard deviations)."""
    g = torch.Generator().manual_seed(7000 + 13 * B + T + C)
    tail = slice(max(T - 32, 0), T)
    if kind == 'cancellation':                       # mean 100, spread 0.1: E[x^2] - E[x]^2 would lose every digit of the variance
        x, relu_in = 100 + 0.1 * torch.randn(B, C, T, generator=g), False
        x[B - 1, :, tail] += 1.0
    else:                                            # no ReLU input near zero
        x, relu_in = torch.randn(B, C, T, generator=g), True
        x = torch.sign(x) * (x.abs() + 0.01)
        x[B - 1, :, tail] *= 4.0
        assert float(x.abs().min()) >= 0.01
    keep = torch.ones(B, T)
    for b in range(B):
        keep[b, T - 1 - (37 * b) % T:] = 0           # ragged (row 0: the last frame)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if kind == 'cancellation':
        rv = 0.01 * rv                               # of the size of the batch variance, so that running_var shows what was mixed into it
    dy = torch.randn(B, C, T, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, keep=keep, dy=dy, relu_in=relu_in)


@functools.lru_cache(maxsize=None)
def bn_refs(B, T, kind, C=8, keep=True):
    """(case, float64 yardstick, float32 yardstick) of a BatchNorm case; keep=False: no mask."""
    c = dict(bn_case(B, T, kind, C))
    if not keep:
        c['keep'] = torch.ones(B, T)
    args = (c['x'], c['gamma'], c['beta'], c['rm'], c['rv'], c['keep'], c['dy'], c['relu_in'])
    return c, bn_reference(*args, torch.float64), bn_restated(*args, torch.float32)


# ----------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU + residual
# ----------------------------------------------------------------------------------------------------------------------------------------
def gn_reference(x, gamma, beta, res, dy, G, dtype, relu=True):
    """y = res + relu(group_norm(x)) and its gradients under L = sum(y dy) (aten); res=None and relu=False drop their terms."""
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.group_norm(x, G, gamma, beta, EPS)
    y = F.relu(y) if relu else y
    if res is not None:
        res = res.to(dtype).clone().requires_grad_(True)
        y = res + y
    (y * dy.to(dtype)).sum().backward()
    out = {'y': y.detach(), 'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad}
    if res is not None:
        out['dres'] = res.grad
    return out


def _gn_stats(x, G):
    B, C, T = x.shape
    xg = x.reshape(B, G, -1)
    n = xg.shape[2]
    mean = xg.sum(2) / n
    e = xg - mean[:, :, None]
    var = (e * e).sum(2) / n
    rstd = 1 / torch.sqrt(var + EPS)
    return (e * rstd[:, :, None]).reshape(B, C, T), rstd, n


def gn_restated(x, gamma, beta, res, dy, G, dtype, relu=True):
    """The same from elementary ops in `dtype`, gradients by autograd."""
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    xh, _, _ = _gn_stats(x, G)
    y = xh * gamma[None, :, None] + beta[None, :, None]
    y = F.relu(y) if relu else y
    if res is not None:
        res = res.to(dtype).clone().requires_grad_(True)
        y = res + y
    (y * dy.to(dtype)).sum().backward()
    out = {'y': y.detach(), 'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad}
    if res is not None:
        out['dres'] = res.grad
    return out


def gn_backward_manual(x, gamma, beta, dy, G, dtype, relu=True, bug=None):
    """dx / dgamma / dbeta written out the way k_pe_gn_bwd sums them: per channel a = sum_t gz xhat and b = sum_t gz (gz = dy (z > 0)), per
    (utterance, group) m1 = sum_c gamma b / n and m2 = sum_c gamma a / n, dx = rstd (gz gamma - m1 - xhat m2).  bug: 'utt0' (dgamma / dbeta
    from utterance 0 only), 'wave0' (the group sums over the channels c % 4 == 0 of the group only: one wave's share)."""
    x, gamma, beta, dy = (t.to(dtype) for t in (x, gamma, beta, dy))
    B, C, T = x.shape
    cg = C // G
    xh, rstd, n = _gn_stats(x, G)
    gz = dy * ((xh * gamma[None, :, None] + beta[None, :, None]) > 0).to(dtype) if relu else dy
    a, b = (gz * xh).sum(2), gz.sum(2)                                   # [B,C]
    own = ((torch.arange(C) % cg) % 4 == 0).to(dtype) if bug == 'wave0' else torch.ones(C, dtype=dtype)
    m1 = (gamma * b * own).reshape(B, G, cg).sum(2) / n                  # [B,G]
    m2 = (gamma * a * own).reshape(B, G, cg).sum(2) / n
    per_c = lambda m: m.repeat_interleave(cg, 1)[:, :, None]             # [B,G] -> [B,C,1]
    dx = per_c(rstd) * (gz * gamma[None, :, None] - per_c(m1) - xh * per_c(m2))
    if bug == 'utt0':
        a, b = a[:1], b[:1]
    return {'dx': dx, 'dgamma': a.sum(0), 'dbeta': b.sum(0)}


def gn_repair(x, gamma, beta, G):
    """Moves the x whose float64 pre-ReLU value is within KINK of zero away from it.  Returns (x, smallest |v|, rounds used)."""
    x = x.clone()
    for rounds in range(21):
        v = F.group_norm(x.double(), G, gamma.double(), beta.double(), EPS)
        near = v.abs() < KINK
        if not bool(near.any()):
            return x, float(v.abs().min()), rounds
        if rounds < 20:
            step = 0.05 * torch.where(v >= 0, 1.0, -1.0) * torch.where(gamma >= 0, 1.0, -1.0).double()[None, :, None]
            x = torch.where(near, x + step.float(), x)
    raise AssertionError(f'{int(near.sum())} pre-ReLU values stay within {KINK} of zero')


@functools.lru_cache(maxsize=None)
def gn_case(B, C, G, T, offset=False):
    """Seeded inputs [B,C,T] of a GroupNorm case (seed 100, the recipe of test_group_norm_backward_operator; offset: x = 100 + 0.1 N), repaired."""
    g = torch.Generator().manual_seed(100)
    x = 100 + 0.1 * torch.randn(B, C, T, generator=g) if offset else torch.randn(B, C, T, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    res, dy = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
    x, vmin, rounds = gn_repair(x, gamma, beta, G)
    return dict(x=x, gamma=gamma, beta=beta, res=res, dy=dy, vmin=vmin, rounds=rounds)


@functools.lru_cache(maxsize=None)
def gn_refs(B, C, G, T, offset=False, plain=False):
    """(case, float64 yardstick, float32 yardstick); plain: relu=False and no residual."""
    c = gn_case(B, C, G, T, offset)
    args = (c['x'], c['gamma'], c['beta'], None if plain else c['res'], c['dy'], G)
    return c, gn_reference(*args, torch.float64, relu=not plain), gn_restated(*args, torch.float32, relu=not plain)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the pitch loss
# ----------------------------------------------------------------------------------------------------------------------------------------
W_UV, W_F0 = 1.3, 0.7                            # L = W_UV uv + W_F0 f0 is what the gradient is taken of


def f0_hp(pitch_loss='l1', use_uv=True):
    return dict(PH.HP, pitch_loss=pitch_loss, use_uv=use_uv, lambda_f0=0.7 if pitch_loss == 'l2' else 1.0, lambda_uv=1.5)


def f0_reference(pred, f0, uv, nonpadding, hp, dtype):
    """pe_train_helpers.f0_losses (torch's own BCE) and d L / d pred."""
    p = pred.to(dtype).clone().requires_grad_(True)
    losses = PH.f0_losses(p, f0.to(dtype), uv.to(dtype), nonpadding.to(dtype), hp)
    (W_UV * losses.get('uv', 0) + W_F0 * losses['f0']).backward()
    return {**{k: v.detach() for k, v in losses.items()}, 'dpred': p.grad}


def f0_restated(pred, f0, uv, nonpadding, hp, dtype, bug=None):
    """add_f0_loss from elementary ops in `dtype`: BCE as max(x, 0) - x z + log1p(exp(-|x|)).  bug: 'drop65536' (the frames from flat index
    65 536 on missing from every sum: a grid that does not stride), 'all_frames' (the f0 term without its (uv == 0) factor)."""
    p = pred.to(dtype).clone().requires_grad_(True)
    f0, uv, w = f0.to(dtype), uv.to(dtype), nonpadding.to(dtype)
    if bug == 'drop65536':
        w = w * (torch.arange(w.numel()).view(w.shape) < F0_FWD_FRAMES).to(dtype)
    losses = {}
    if hp['use_uv']:
        xl = p[:, :, 1]
        bce = xl.clamp_min(0) - xl * uv + torch.log1p(torch.exp(-xl.abs()))
        losses['uv'] = (bce * w).sum() / w.sum() * hp['lambda_uv']
        if bug != 'all_frames':
            w = w * (uv == 0).to(dtype)
    d = p[:, :, 0] - f0
    losses['f0'] = ((d.abs() if hp['pitch_loss'] == 'l1' else d * d) * w).sum() / w.sum() * hp['lambda_f0']
    (W_UV * losses.get('uv', 0) + W_F0 * losses['f0']).backward()
    return {**{k: v.detach() for k, v in losses.items()}, 'dpred': p.grad}


@functools.lru_cache(maxsize=None)
def f0_case(B, T, Cp=2):
    """Seeded pitch-loss inputs: pred [B,T,Cp] (log2 f0, the voicing logit, Cp - 2 channels the loss must ignore), the +-40 logits of the
    overflow-safe BCE form, row 1 entirely unvoiced, a ragged nonpadding; the frames from flat index 65 536 on are 1.5 off in f0."""
    g = torch.Generator().manual_seed(5 + B + T)
    pred = torch.stack([7.5 + 0.5 * torch.randn(B, T, generator=g), 2 * torch.randn(B, T, generator=g)]
                       + [torch.randn(B, T, generator=g) for _ in range(Cp - 2)], -1)
    pred[0, 3, 1], pred[1, 4, 1], pred[2, 5, 1], pred[2, 6, 1] = 40.0, -40.0, 40.0, -40.0
    f0, uv = 7.5 + 0.5 * torch.randn(B, T, generator=g), (torch.rand(B, T, generator=g) < 0.3).float()
    uv[1] = 1.0
    uv[0, 3], uv[1, 4], uv[2, 5], uv[2, 6] = 1.0, 1.0, 0.0, 0.0
    pred[:, :, 0] += 1.5 * (torch.arange(B * T).view(B, T) >= F0_FWD_FRAMES).float()
    nonpadding = torch.ones(B, T)
    for b in range(1, B):                            # the last row is the longest of them: the frames of a second grid pass stay live
        nonpadding[b, T - (T * (5 + 7 * (B - 1 - b))) // 100:] = 0
    return dict(pred=pred, f0=f0, uv=uv, nonpadding=nonpadding)


@functools.lru_cache(maxsize=None)
def f0_refs(B, T, Cp=2, pitch_loss='l1', use_uv=True):
    c, hp = f0_case(B, T, Cp), f0_hp(pitch_loss, use_uv)
    args = (c['pred'], c['f0'], c['uv'], c['nonpadding'], hp)
    return c, hp, f0_reference(*args, torch.float64), f0_restated(*args, torch.float32)


# ----------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm in eval mode: y = (x a + b) keep
# ----------------------------------------------------------------------------------------------------------------------------------------
def affine_case(B, C, T, keep):
    """x [B,C,T], a / b [C] as Prenet derives them from an eval-mode BatchNorm1d, keep [B,T] (ragged per row) or None."""
    g = torch.Generator().manual_seed(31 + B + C + T)
    x = torch.randn(B, C, T, generator=g) * 2 + 0.5
    a = (1 + 0.1 * torch.randn(C, generator=g)) / torch.sqrt(0.5 + torch.rand(C, generator=g) + EPS)
    b = 0.1 * torch.randn(C, generator=g) - 0.3 * torch.randn(C, generator=g) * a
    k = None
    if keep is not None:
        k = torch.ones(B, T)
        for r in range(B):
            k[r, T - 1 - (37 * r) % T:] = 0
    return x, a, b, k


def affine_reference(x, a, b, keep):
    """(float64 value, per-element bound): |fl(fl(x a) + b) - (x a + b)| <= u |x a| + u (1 + u) |x a + b| < 4 u (|x a| + |b|), fused or not;
    the mask is 0 or 1 and multiplies exactly."""
    xa = x.double() * a.double()[None, :, None]
    want = xa + b.double()[None, :, None]
    tol = 4 * U * (xa.abs() + b.double().abs()[None, :, None])
    if keep is not None:
        want = want * keep.double()[:, None, :]
    return want, tol
