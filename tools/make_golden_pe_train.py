"""Developer tool (CPU, needs the reference checkout): writes tests/golden/pe_train_ref.npz from the REFERENCE'S OWN PitchExtractor in train mode.

    python tools/make_golden_pe_train.py [--reference /path/to/reference] [--seed N]        (default: $DIFFSINGER_REFERENCE, seed 407)

modules/fastspeech/pe.py is imported from the reference tree under the shipped opencpop e2e config with the hparams of
tests/pe_train_helpers.HP on top (hidden_size 64: the file stays small), every nn.Dropout.p set to 0, the seeded state of
oracle.pe_oracle.synth_extractor_params(hp, seed + 1000), mel = synth_mel(3, 47, seed), f0 ~ 7.5 + 0.5 N(0,1), uv ~ Bernoulli(0.3).  One training
step: forward in train mode (BatchNorm1d on batch statistics, buffers updated), the loss of PitchExtractionTask.add_pitch_loss (tasks/tts/pe.py:
146-155 -> add_f0_loss, tasks/tts/fs2.py:254-269; the task module itself needs librosa / matplotlib / the data pipeline to import, so its two
expressions are evaluated on the module's output by tests/pe_train_helpers.f0_losses), backward.

Stored (data only): pitch_pred, both loss values ('loss/uv', 'loss/f0'), every parameter gradient ('grad/<name>'), the three BatchNorm layers'
updated running_mean / running_var / num_batches_tracked ('running/<name>'), per tensor the fp32 reference's deviation from the float64
restatement of tests/pe_train_helpers.py ('dev/<name>': max|x32 - x64| / max|x64|), hp, the seed and 'relu_min_ratio'.

A seed is only recorded when every ReLU input of the step is well away from its kink: |v64| >= 8 |v32_ref - v64| at every ReLU input (10
layers, 90 240 values) and no sign disagreement - asserted here; the smallest ratio is stored."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pe_train_helpers as PH  # noqa: E402

CONFIG = 'usr/configs/midi/e2e/opencpop/ds100_adj_rel.yaml'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    ap.add_argument('--seed', type=int, default=PH.CASE['seed'])
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_pe_train: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    os.environ['DIFFSINGER_REFERENCE'] = args.reference
    from oracle import pe_oracle as PO
    from oracle.ref_driver import Reference
    hp = dict(PH.HP)
    Reference(CONFIG, overrides=hp)
    from modules.fastspeech.pe import PitchExtractor
    B, T, seed = PH.CASE['B'], PH.CASE['T'], args.seed
    m = PitchExtractor().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    state, mel, f0, uv = PH.case_inputs(hp, B, T, seed)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v) for k, v in PO.extractor_shapes(hp).items()}
    m.load_state_dict(state, strict=True)
    relu32 = []
    for mod in m.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.register_forward_pre_hook(lambda _m, inp: relu32.append(inp[0].detach()))
    out = m(mel)
    pitch_pred = out['pitch_pred']
    assert pitch_pred.dtype == torch.float32
    nonpadding = (mel.abs().sum(-1) > 0).float()
    losses = PH.f0_losses(pitch_pred, f0, uv, nonpadding, hp)
    sum(losses.values()).backward()
    grads = {k: v.grad.detach().clone() for k, v in m.named_parameters()}
    new_state = m.state_dict()
    running = {k: new_state[k].detach().clone() for k in new_state if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}

    want = PH.training_step(state, hp, mel, f0, uv, torch.float64)
    assert len(relu32) == len(want['relu']) == 10, (len(relu32), len(want['relu']))
    assert sum(v.numel() for v in relu32) == 10 * hp['hidden_size'] * B * T
    ratio, flips = PH.relu_condition(relu32, want['relu'])
    assert flips == 0 and ratio >= PH.RELU_MARGIN, f'seed {seed}: smallest |v64| / |v32 - v64| = {ratio:.3g}, {flips} sign disagreements - try another seed'
    assert set(grads) == set(want['grad']), set(grads) ^ set(want['grad'])
    dev = {'pitch_pred': PH.rel_err(pitch_pred.detach(), want['pitch_pred']), 'loss/uv': PH.rel_err(losses['uv'].detach(), want['uv']),
           'loss/f0': PH.rel_err(losses['f0'].detach(), want['f0'])}
    dev.update({'grad/' + k: PH.rel_err(v, want['grad'][k]) for k, v in grads.items()})
    for k, v in running.items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(want['running'][k]) == 8
        else:
            dev['running/' + k] = PH.rel_err(v, want['running'][k])
    worst = max(dev.values())
    assert worst < 1e-4, f'the float64 restatement and the reference disagree: {max(dev, key=dev.get)} {worst:.3e}'

    arrays = {'pitch_pred': pitch_pred.detach().numpy(), 'loss/uv': losses['uv'].detach().numpy(), 'loss/f0': losses['f0'].detach().numpy(),
              'hp': np.array(repr(hp)), 'seed': np.int64(seed), 'B': np.int64(B), 'T': np.int64(T), 'relu_min_ratio': np.float64(ratio)}
    arrays.update({'grad/' + k: v.numpy() for k, v in grads.items()})
    arrays.update({'running/' + k: v.numpy() for k, v in running.items()})
    arrays.update({'dev/' + k: np.float64(v) for k, v in dev.items()})
    np.savez_compressed(PH.FIXTURE, **arrays)
    print(f"{PH.FIXTURE}: seed {seed}, losses uv {float(losses['uv'].detach()):.6f} f0 {float(losses['f0'].detach()):.6f}, smallest ReLU ratio {ratio:.1f}, "
          f"fp32 deviation pitch_pred {dev['pitch_pred']:.3e}, worst {max(dev, key=dev.get)} {worst:.3e}, {os.path.getsize(PH.FIXTURE)} bytes")


if __name__ == '__main__':
    main()
