"""Developer tool (CPU, needs the reference checkout): writes tests/golden/pwg_disc_ref.npz from the REFERENCE'S OWN module code.

    python tools/make_golden_pwg_disc.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE)

modules/parallel_wavegan/models/parallel_wavegan.py is imported from the reference tree (its import chain reaches layers/pqmf.py, which wants
the pre-1.13 name scipy.signal.kaiser: aliased here as oracle/make_golden_pwg.py does; librosa / pycwt are not on this path and are stubbed).

Stored (data only):
  * ParallelWaveGANDiscriminator(layers=4), other arguments at their defaults, with the seeded O(1) state of tests/pwg_disc_helpers.synth_state:
    the full state ('state/<key>'), x [2][1][1061], and the module's float32 CPU output ('out'), dL/dx ('dx') and every parameter gradient
    ('grad/<key>') under L = mean((p - 1)^2);
  * 'keys_json': {variant: [[key, shape], ...]} of the DEFAULT 10-layer module for weight norm x bias (variants 'wn1_b1', 'wn1_b0', 'wn0_b1',
    'wn0_b0'; the plain form is the module after its own remove_weight_norm()) - names and shapes only, no values.
The float64 restatement of tests/pwg_disc_helpers.py must reproduce the recorded numbers within its rule before anything is written."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pwg_disc_helpers as DH  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'pwg_disc_ref.npz')
LAYERS, SEED, SHAPE = 4, 20240607, (2, 1, 1061)


def reference_class(root):
    sys.dont_write_bytecode = True
    for n in ('librosa', 'pycwt'):
        sys.modules.setdefault(n, types.ModuleType(n))
    import scipy.signal
    import scipy.signal.windows
    if not hasattr(scipy.signal, 'kaiser'):
        scipy.signal.kaiser = scipy.signal.windows.kaiser
    sys.path.insert(0, root)
    from modules.parallel_wavegan.models.parallel_wavegan import ParallelWaveGANDiscriminator
    return ParallelWaveGANDiscriminator


def check_against_float64(state, x, out, dx, grads, slope):
    """the recorded float32 numbers within the rule of the float64 restatement (own masks, bounds propagated from x)"""
    ws, bs = DH.plain_params(state, LAYERS)
    x64 = DH.d64(x)
    f = DH.forward64(x64, ws, bs, slope)
    worst = float(((DH.d64(out) - f['p']).abs() - f['e_p']).max())
    gp, e_gp = DH.generator_gp(f['p'], f['e_p'])
    bw = DH.backward64(gp, e_gp, x64, ws, f['act'], slope, f['e_act'])
    worst = max(worst, float(((DH.d64(dx) - bw['dx'][0]).abs() - bw['dx'][1]).max()))
    for i in range(LAYERS):
        pre = f'conv_layers.{2 * i}.'
        (gg, bg), (gv, bv) = DH.weight_norm_grads64(DH.d64(state[pre + 'weight_g']), DH.d64(state[pre + 'weight_v']), *bw['dw'][i])
        for key, val, bound in ((pre + 'weight_g', gg, bg), (pre + 'weight_v', gv, bv), (pre + 'bias', *bw['db'][i])):
            worst = max(worst, float(((DH.d64(grads[key]) - val).abs() - bound).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_pwg_disc: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    Ref = reference_class(args.reference)
    keys = {}
    for wn in (1, 0):
        for b in (1, 0):
            m = Ref(bias=bool(b), use_weight_norm=True)
            if not wn:
                m.remove_weight_norm()
            keys[f'wn{wn}_b{b}'] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    m = Ref(layers=LAYERS)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == DH.module_shapes(LAYERS), set(shapes) ^ set(DH.module_shapes(LAYERS))
    state = DH.synth_state(shapes, SEED)
    m.load_state_dict(state, strict=True)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(SEED + 1))
    xg = x.clone().requires_grad_(True)
    p = m(xg)
    loss = torch.mean((p - 1) ** 2)
    loss.backward()
    assert p.dtype == torch.float32
    grads = {k: v.grad.detach().clone() for k, v in m.named_parameters()}
    slope = 0.2
    worst = check_against_float64(state, x, p.detach(), xg.grad, grads, slope)
    assert worst <= 0.0, f'the float64 restatement misses the reference by {worst:.3e} beyond its bound'
    arrays = {'x': x.numpy(), 'out': p.detach().numpy(), 'dx': xg.grad.numpy(), 'layers': np.int64(LAYERS), 'slope': np.float64(slope),
              'keys_json': np.array(json.dumps(keys))}
    arrays.update({'state/' + k: v.numpy() for k, v in state.items()})
    arrays.update({'grad/' + k: v.numpy() for k, v in grads.items()})
    np.savez(OUT, **arrays)
    print(f'{OUT}: loss {float(loss.detach()):.6f}, max |p| {float(p.detach().abs().max()):.3f}, max |dx| {float(xg.grad.abs().max()):.3e}, '
          f'float64 restatement within its bound (worst margin {worst:.3e}), {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
