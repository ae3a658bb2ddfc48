"""Developer tool (CPU, needs the reference checkout): writes tests/golden/voc_optim_ref.npz from the REFERENCE'S OWN optimiser.

    python tools/make_golden_voc_optim.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE)

modules/parallel_wavegan/optimizers/radam.py is loaded by file path (its package imports the models, which this tool has no use for).  Nothing of
the reference's program text is copied; the fixture holds data only.

Recorded, float32 on the CPU: tests/voc_optim_helpers.inputs(FIXTURE_SIZES, FIXTURE_SEED) - five tensors of 1, 3, 5, 64 and 1027 elements, eight
gradients each - as 'p0/<i>' and 'g/<step>/<i>', and for each of the two settings of voc_optim_helpers.SETTINGS (betas (0.9, 0.999) without and
(0.8, 0.99) with weight decay) the parameters and both moments after every step: '<setting>/p|m|v/<step>/<i>'."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import voc_optim_helpers as OH  # noqa: E402


def reference_radam(root):
    path = os.path.join(root, 'modules', 'parallel_wavegan', 'optimizers', 'radam.py')
    spec = importlib.util.spec_from_file_location('reference_radam', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.RAdam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_voc_optim: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    RAdam = reference_radam(args.reference)
    p0, grads = OH.inputs(OH.FIXTURE_SIZES, OH.FIXTURE_SEED)
    arrays = {f'p0/{i}': t.numpy() for i, t in enumerate(p0)}
    arrays.update({f'g/{s}/{i}': g.numpy() for s, gs in enumerate(grads) for i, g in enumerate(gs)})
    for name, hp in OH.SETTINGS.items():
        params = [torch.nn.Parameter(t.clone()) for t in p0]
        opt = RAdam(params, **hp)
        for s, gs in enumerate(grads):
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()
            for i, p in enumerate(params):
                st = opt.state[p]
                assert st['step'] == s + 1
                arrays[f'{name}/p/{s}/{i}'] = p.detach().numpy().copy()
                arrays[f'{name}/m/{s}/{i}'] = st['exp_avg'].numpy().copy()
                arrays[f'{name}/v/{s}/{i}'] = st['exp_avg_sq'].numpy().copy()
    np.savez_compressed(OH.FIXTURE, **arrays)
    size = os.path.getsize(OH.FIXTURE)
    assert size <= 600 * 1000, size
    print(f'{OH.FIXTURE}: {size} bytes')


if __name__ == '__main__':
    main()
