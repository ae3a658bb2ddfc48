"""Developer tool (CPU, needs the reference checkout): writes tests/golden/hifigan_disc_ref.npz from the REFERENCE'S OWN module code.

    python tools/make_golden_hifigan_disc.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE)

modules.hifigan.hifigan.MultiScaleDiscriminator, feature_loss, generator_loss and discriminator_loss are imported from the reference tree as
tools/make_golden_hifigan_train.py imports its module (scipy.signal.kaiser aliased, librosa / pycwt stubbed; hparams['hop_size'] set).  Nothing of
the reference's program text is copied; the fixture holds data only.

The state is tests/hifigan_disc_helpers.fixture_inputs(): 30 M floats that cannot be committed - the seed and the recipe regenerate it, and the
fixture records the key list and the shapes.  Recorded under 'eval/' and 'train/' (one call each, B = 1, T = 300, float32 on the CPU):

  * 'y', 'y_hat' (once); the six outputs 'r0'..'r2', 'g0'..'g2'; 'losses' = feature_loss, generator_loss, r_loss, g_loss;
  * 'dy_hat' and, per parameter, a subsample of the gradient of L = feature_loss + generator_loss + r_loss + g_loss ('grad/<key>');
  * per feature map a subsample ('fr<i>_<l>', 'fg<i>_<l>'); the subsample is hifigan_disc_helpers.sample_index(numel, seed + position): at most
    256 seeded flat indices, stored beside the values ('idx/...');
  * 'u<l>': discriminator 0's weight_u after the call.

The file must stay under 600 KB."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hifigan_disc_helpers as DH  # noqa: E402


def reference_module(root):
    sys.dont_write_bytecode = True
    for n in ('librosa', 'pycwt'):
        sys.modules.setdefault(n, types.ModuleType(n))
    import scipy.signal
    import scipy.signal.windows
    if not hasattr(scipy.signal, 'kaiser'):
        scipy.signal.kaiser = scipy.signal.windows.kaiser
    sys.path.insert(0, root)
    from utils.hparams import hparams
    hparams['hop_size'] = DH.HOP
    import modules.hifigan.hifigan as ref
    return ref


def record(ref, state, y, y_hat, training, pos):
    m = ref.MultiScaleDiscriminator()
    m.load_state_dict(state, strict=True)
    m.train(training)
    yh = y_hat.clone().requires_grad_(True)
    rs, gs, frs, fgs = m(y, yh)
    fl = ref.feature_loss(frs, fgs)
    gen = ref.generator_loss(gs)
    rl, gl = ref.discriminator_loss(rs, gs)
    (fl + gen + rl + gl).backward()
    out = {'losses': np.array([float(fl), float(gen), float(rl), float(gl)], np.float64), 'dy_hat': yh.grad.numpy()}
    idx = {}

    def sub(name, t):
        i = DH.sample_index(t.numel(), DH.FIXTURE_SEED + pos[0])
        pos[0] += 1
        idx[name] = i.astype(np.int32)
        out[name] = t.detach().reshape(-1).numpy()[i]
    for i in range(3):
        out[f'r{i}'], out[f'g{i}'] = rs[i].detach().numpy(), gs[i].detach().numpy()
        for l in range(DH.N):
            sub(f'fr{i}_{l}', frs[i][l])
            sub(f'fg{i}_{l}', fgs[i][l])
    for k, p in sorted(m.named_parameters()):
        sub('grad/' + k, p.grad)
    for l, p in enumerate(DH.prefixes(0)):
        out[f'u{l}'] = m.state_dict()[p + 'weight_u'].numpy().copy()
    return out, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_hifigan_disc: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    ref = reference_module(args.reference)
    state, y, y_hat = DH.fixture_inputs()
    shapes = {k: list(v.shape) for k, v in ref.MultiScaleDiscriminator().state_dict().items()}
    assert {k: tuple(v) for k, v in shapes.items()} == DH.module_shapes(), 'the helper restates other keys / shapes than the reference has'
    arrays = {'y': y.numpy(), 'y_hat': y_hat.numpy()}
    for mode in ('eval', 'train'):
        pos = [0]                                               # both modes use the same index sets
        out, idx = record(ref, state, y, y_hat, mode == 'train', pos)
        arrays.update({f'{mode}/{k}': v for k, v in out.items()})
        if mode == 'eval':
            arrays.update({f'idx/{k}': v for k, v in idx.items()})
        print(mode, 'losses', out['losses'])
    arrays['meta_json'] = np.array(json.dumps({'keys': list(shapes), 'shapes': [shapes[k] for k in shapes], 'seed': DH.FIXTURE_SEED,
                                               'B': DH.FIXTURE_B, 'T': DH.FIXTURE_T, 'hop_size': DH.HOP, 'samples': DH.FIXTURE_SAMPLES}))
    np.savez_compressed(DH.FIXTURE, **arrays)
    size = os.path.getsize(DH.FIXTURE)
    assert size <= 600 * 1000, size
    print(f'{DH.FIXTURE}: {size} bytes')


if __name__ == '__main__':
    main()
