"""Test infrastructure of the PitchExtractor TRAINING path: the case of tests/golden/pe_train_ref.npz and a functional torch restatement of
PitchExtractionTask's training step (modules/fastspeech/pe.py in train mode + tasks/tts/pe.py:128-155, tasks/tts/fs2.py:254-269) that runs in
float64 (the yardstick) or float32 (the CPU reference whose own error sets the tolerance) under torch autograd:

    Prenet          F.conv1d -> F.relu -> F.batch_norm(training=True) -> * nonpadding, x3, out_proj          (batch statistics: every frame of
                    the batch counts, padding frames included - the reference masks AFTER the norm)
    ConvStacks      oracle.pe_oracle.conv_stacks
    PitchPredictor  oracle.fs2_oracle.pitch_predictor (dropout 0)
    loss            uv = sum(BCEWithLogits(p1, uv) np) / sum(np) lambda_uv ; f0 = sum(|p0 - f0| np (uv == 0)) / sum(np (uv == 0)) lambda_f0

The error of a tensor X against its float64 value is max|X - X64| / max|X64| (rel_err).  The tolerance rule of the GPU tests (bound): at most 4 x
the fp32 CPU reference's error on the same tensor, with a floor of 2e-6 - the MFMA and tree-reduction summation orders differ from aten's by
O(1) factors in rounding error, a wrong formula (biased / unbiased variance, a missing mean term, tail columns counted, the mask before the
statistics) is off by 1e-3 or more.

ReLU kinks: a ReLU input whose sign differs between two correct fp32 evaluations changes the gradients discontinuously, so a case is only
usable when every ReLU input is well away from zero: |v64| >= 8 |v32 - v64| everywhere and no sign disagreement (relu_condition)."""
import contextlib
import os

import torch
import torch.nn.functional as F

from oracle import fs2_oracle as FO
from oracle import pe_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'pe_train_ref.npz')
HP = dict(hidden_size=64, predictor_hidden=-1, predictor_kernel=5, ffn_padding='SAME', pitch_type='frame', use_uv=True, pitch_norm='log',
          pitch_loss='l1', lambda_f0=1.0, lambda_uv=1.0)
CASE = dict(B=3, T=47, seed=407)
BUFFERS = ('running_mean', 'running_var', 'num_batches_tracked', '_float_tensor')
FLOOR, FACTOR, RELU_MARGIN = 2e-6, 4.0, 8.0


def synth_targets(B, T, seed):
    """f0 ~ 7.5 + 0.5 N(0,1) (log2 Hz), uv ~ Bernoulli(0.3), both [B,T] fp32."""
    g = torch.Generator().manual_seed(seed + 2000)
    f0 = 7.5 + 0.5 * torch.randn(B, T, generator=g)
    uv = (torch.rand(B, T, generator=g) < 0.3).float()
    return f0, uv


def is_param(key):
    return not key.endswith(BUFFERS)


def rel_err(x, x64):
    x, x64 = torch.as_tensor(x).double(), torch.as_tensor(x64).double()
    return float((x - x64).abs().max() / x64.abs().max().clamp_min(1e-300))


def bound(ref_err):
    return max(FACTOR * float(ref_err), FLOOR)


@contextlib.contextmanager
def record_relu(store):
    """Every F.relu input of the restatement (the oracle modules call torch.nn.functional.relu through the module object)."""
    orig = F.relu

    def relu(x, *a, **k):
        store.append(x.detach())
        return orig(x, *a, **k)
    F.relu = relu
    try:
        yield store
    finally:
        F.relu = orig


def relu_condition(relu_a, relu_64):
    """(smallest |v64| / |va - v64| over every ReLU input, number of sign disagreements)."""
    assert len(relu_a) == len(relu_64)
    worst, flips = float('inf'), 0
    for a, b in zip(relu_a, relu_64):
        a, b = a.double(), b.double()
        diff = (a - b).abs()
        ratio = torch.where(diff > 0, b.abs() / diff.clamp_min(1e-300), torch.full_like(b, float('inf')))
        worst = min(worst, float(ratio.min()))
        flips += int(((a > 0) != (b > 0)).sum())
    return worst, flips


def prenet_train(p, pre, x_btc, running, momentum=0.1, eps=1e-5, n_layers=3, kernel=5):
    """Prenet.forward (pe.py:23-41) in train mode; `running` receives the updated buffers under the state dict's names."""
    keep = 1 - x_btc.abs().sum(-1).eq(0).to(x_btc.dtype)[:, None, :]
    x = x_btc.transpose(1, 2)
    for l in range(n_layers):
        k = f'{pre}layers.{l}.'
        x = F.relu(F.conv1d(x, p[k + '0.weight'], p[k + '0.bias'], padding=kernel // 2))
        rm, rv = p[k + '2.running_mean'].detach().clone(), p[k + '2.running_var'].detach().clone()
        x = F.batch_norm(x, rm, rv, p[k + '2.weight'], p[k + '2.bias'], True, momentum, eps) * keep
        running[k + '2.running_mean'], running[k + '2.running_var'] = rm, rv
        running[k + '2.num_batches_tracked'] = p[k + '2.num_batches_tracked'] + 1
    x = F.linear(x.transpose(1, 2), p[pre + 'out_proj.weight'], p[pre + 'out_proj.bias'])
    return x * keep.transpose(1, 2)


def f0_losses(pitch_pred, f0, uv, nonpadding, hp):
    """add_f0_loss (tasks/tts/fs2.py:254-269), pitch_loss l1 / l2."""
    losses = {}
    if hp['use_uv']:
        losses['uv'] = (F.binary_cross_entropy_with_logits(pitch_pred[:, :, 1], uv, reduction='none') * nonpadding).sum() / nonpadding.sum() * hp['lambda_uv']
        nonpadding = nonpadding * (uv == 0).to(nonpadding.dtype)
    d = pitch_pred[:, :, 0] - f0
    losses['f0'] = ((d.abs() if hp['pitch_loss'] == 'l1' else d * d) * nonpadding).sum() / nonpadding.sum() * hp['lambda_f0']
    return losses


def training_step(state, hp, mel, f0, uv, dtype=torch.float64):
    """One training step of the restatement in `dtype` -> {'pitch_pred', 'uv', 'f0', 'grad': {name: tensor}, 'running': {name: tensor},
    'relu': [every ReLU input, in order]}."""
    p = {}
    for k, v in state.items():
        if v.is_floating_point():
            p[k] = v.detach().to(dtype).clone().requires_grad_(is_param(k))
        else:
            p[k] = v.clone()
    mel, f0, uv = mel.to(dtype), f0.to(dtype), uv.to(dtype)
    running, relu = {}, []
    with record_relu(relu):
        h = prenet_train(p, 'mel_prenet.', mel, running)
        h = PO.conv_stacks(p, 'mel_encoder.', h, 2)
        pitch_pred = FO.pitch_predictor(p, 'pitch_predictor.', h, 5, hp['predictor_kernel'])
    nonpadding = (mel.abs().sum(-1) > 0).to(dtype)
    losses = f0_losses(pitch_pred, f0, uv, nonpadding, hp)
    sum(losses.values()).backward()
    return {'pitch_pred': pitch_pred.detach(), 'uv': losses['uv'].detach(), 'f0': losses['f0'].detach(),
            'grad': {k: v.grad.detach() for k, v in p.items() if v.is_floating_point() and v.requires_grad},
            'running': running, 'relu': relu}


def case_inputs(hp=None, B=None, T=None, seed=None):
    """(state, mel, f0, uv) of a seeded case (default: the fixture's)."""
    hp = HP if hp is None else hp
    B, T, seed = CASE['B'] if B is None else B, CASE['T'] if T is None else T, CASE['seed'] if seed is None else seed
    state = PO.synth_extractor_params(hp, seed + 1000)
    f0, uv = synth_targets(B, T, seed)
    return state, PO.synth_mel(B, T, seed), f0, uv
