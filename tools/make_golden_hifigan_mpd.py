"""Developer tool (CPU, needs the reference checkout): writes tests/golden/hifigan_mpd_ref.npz from the REFERENCE'S OWN module code.

    python tools/make_golden_hifigan_mpd.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE)

modules.hifigan.hifigan.MultiPeriodDiscriminator, feature_loss, generator_loss and discriminator_loss are imported from the reference tree as
tools/make_golden_hifigan_disc.py imports its module.  Nothing of the reference's program text is copied; the fixture holds data only.

The state is tests/hifigan_mpd_helpers.fixture_inputs(): 41 M floats that cannot be committed - the seed and the recipe regenerate it, and the
fixture records the key list and the shapes.  Recorded (one call, B = 1, T = 300, float32 on the CPU):

  * 'y', 'y_hat'; the ten outputs 'r0'..'r4', 'g0'..'g4'; 'losses' = feature_loss, generator_loss, r_loss, g_loss;
  * 'dy_hat' and, per parameter, a subsample of the gradient of L = feature_loss + generator_loss + r_loss + g_loss ('grad/<key>');
  * per feature map a subsample ('fr<i>_<l>', 'fg<i>_<l>'); the subsample is hifigan_disc_helpers.sample_index(numel, seed + position): at most
    256 seeded flat indices, stored beside the values ('idx/...').

The file must stay under 600 KB."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from tests import hifigan_mpd_helpers as MH  # noqa: E402
from make_golden_hifigan_disc import reference_module  # noqa: E402


def record(ref, state, y, y_hat):
    m = ref.MultiPeriodDiscriminator()
    m.load_state_dict(state, strict=True)
    yh = y_hat.clone().requires_grad_(True)
    rs, gs, frs, fgs = m(y, yh)
    fl = ref.feature_loss(frs, fgs)
    gen = ref.generator_loss(gs)
    rl, gl = ref.discriminator_loss(rs, gs)
    (fl + gen + rl + gl).backward()
    out = {'losses': np.array([float(fl), float(gen), float(rl), float(gl)], np.float64), 'dy_hat': yh.grad.numpy()}
    idx, pos = {}, [0]

    def sub(name, t):
        i = MH.sample_index(t.numel(), MH.FIXTURE_SEED + pos[0], MH.FIXTURE_SAMPLES)
        pos[0] += 1
        idx[name] = i.astype(np.int32)
        out[name] = t.detach().reshape(-1).numpy()[i]
    for i in range(len(MH.PERIODS)):
        out[f'r{i}'], out[f'g{i}'] = rs[i].detach().numpy(), gs[i].detach().numpy()
        for l in range(MH.N):
            sub(f'fr{i}_{l}', frs[i][l])
            sub(f'fg{i}_{l}', fgs[i][l])
    for k, p in sorted(m.named_parameters()):
        sub('grad/' + k, p.grad)
    return out, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_hifigan_mpd: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    ref = reference_module(args.reference)
    state, y, y_hat = MH.fixture_inputs()
    shapes = {k: list(v.shape) for k, v in ref.MultiPeriodDiscriminator().state_dict().items()}
    assert {k: tuple(v) for k, v in shapes.items()} == MH.module_shapes(), 'the helper restates other keys / shapes than the reference has'
    arrays = {'y': y.numpy(), 'y_hat': y_hat.numpy()}
    out, idx = record(ref, state, y, y_hat)
    arrays.update(out)
    arrays.update({f'idx/{k}': v for k, v in idx.items()})
    print('losses', out['losses'])
    arrays['meta_json'] = np.array(json.dumps({'keys': list(shapes), 'shapes': [shapes[k] for k in shapes], 'seed': MH.FIXTURE_SEED,
                                               'B': MH.FIXTURE_B, 'T': MH.FIXTURE_T, 'samples': MH.FIXTURE_SAMPLES}))
    np.savez_compressed(MH.FIXTURE, **arrays)
    size = os.path.getsize(MH.FIXTURE)
    assert size <= 600 * 1000, size
    print(f'{MH.FIXTURE}: {size} bytes')


if __name__ == '__main__':
    main()
