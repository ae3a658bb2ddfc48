"""Developer tool (CPU, needs the reference checkout): writes tests/golden/pwg_train_ref.npz from the REFERENCE'S OWN module code.

    python tools/make_golden_pwg_train.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE)

modules/parallel_wavegan/models/parallel_wavegan.py is imported from the reference tree as tools/make_golden_pwg_disc.py does (scipy.signal.kaiser
aliased, librosa / pycwt stubbed).  Nothing of the reference's program text is copied; the fixture holds data only:

  * ParallelWaveGANGenerator(layers=4, stacks=2, aux_channels=16, upsample_scales [4, 4, 4, 4], weight norm on) with the seeded O(1) state of
    tests/pwg_train_helpers.synth_state rounded to float16 ('state/<key>', stored as float16 without loss: the committed file stays below
    1 MiB); x [2][1][1536] noise, c [2][16][6 + 2 * 2] conditioning, a target waveform;
  * the module's float32 CPU output ('out') and every parameter gradient ('grad/<key>') under L = mean((y - target)^2);
  * 'meta_json': the configuration and the keys whose gradient the reference's autograd leaves at None;
  * 'err/<key>' = max|grad_fp32 - grad_fp64| and 'err_out' = max|out_fp32 - out_fp64| of the reference module itself (its .double() copy).
The float64 restatement of tests/pwg_train_helpers.py must reproduce the recorded numbers before anything is written."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pwg_train_helpers as TH  # noqa: E402

CFG = dict(layers=4, stacks=2, aux=16, scales=[4, 4, 4, 4], ctx=2, bias=True)
SEED, B, FRAMES = 20240612, 2, 6


def reference_class(root):
    sys.dont_write_bytecode = True
    for n in ('librosa', 'pycwt'):
        sys.modules.setdefault(n, types.ModuleType(n))
    import scipy.signal
    import scipy.signal.windows
    if not hasattr(scipy.signal, 'kaiser'):
        scipy.signal.kaiser = scipy.signal.windows.kaiser
    sys.path.insert(0, root)
    from modules.parallel_wavegan.models.parallel_wavegan import ParallelWaveGANGenerator
    return ParallelWaveGANGenerator


def run(module, x, c, target):
    module.zero_grad()
    y = module(x, c)
    torch.mean((y - target) ** 2).backward()
    return y.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in module.named_parameters()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_pwg_train: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    Ref = reference_class(args.reference)
    cfg = TH.config(**CFG)

    def make():
        return Ref(layers=cfg['layers'], stacks=cfg['stacks'], aux_channels=cfg['aux'], aux_context_window=cfg['ctx'],
                   upsample_params={'upsample_scales': list(cfg['scales'])})
    m = make()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == TH.module_shapes(cfg), set(shapes) ^ set(TH.module_shapes(cfg))
    state = {k: v.half().float() for k, v in TH.synth_state(shapes, SEED).items()}     # exactly representable in float16: stored at half the size
    m.load_state_dict(state, strict=True)
    T = FRAMES * int(np.prod(cfg['scales']))
    gen = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(B, 1, T, generator=gen)
    c = torch.randn(B, cfg['aux'], FRAMES + 2 * cfg['ctx'], generator=gen)
    target = 0.5 * torch.randn(B, 1, T, generator=gen)
    out, grads = run(m, x, c, target)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 1, T)
    m64 = make()
    m64.load_state_dict(state, strict=True)
    m64 = m64.double()
    out64, grads64 = run(m64, x.double(), c.double(), target.double())
    none_keys = sorted(k for k, g in grads.items() if g is None)
    assert none_keys == sorted(k for k, g in grads64.items() if g is None)
    err = {k: float((grads[k].double() - grads64[k]).abs().max()) for k in grads if grads[k] is not None}
    err_out = float((out.double() - out64).abs().max())
    # the helper's float64 restatement against the recorded numbers, with the test's own tolerances
    o_h, g_h, dw_h = TH.module_grads(state, x, c, cfg, TH.mse_to(target))
    assert sorted(k for k, g in g_h.items() if g is None) == none_keys, 'the restatement leaves other gradients at None'
    assert float((o_h - out.double()).abs().max()) <= max(4 * err_out, TH.RULE * float(o_h.abs().max()))
    tol = TH.tolerances(state, g_h, dw_h, err)
    worst = 0.0
    for k, t in tol.items():
        e = float((grads[k].double() - g_h[k]).abs().max())
        assert e <= t, f'{k}: the float64 restatement misses the reference by {e:.3e} (tolerance {t:.3e})'
        worst = max(worst, e / t)
    rel = max(err[k] / float(grads64[k].abs().max()) for k in err if k != 'first_conv.weight_v')
    arrays = {'x': x.numpy(), 'c': c.numpy(), 'target': target.numpy(), 'out': out.numpy(), 'err_out': np.float64(err_out),
              'meta_json': np.array(json.dumps({'cfg': CFG, 'none_keys': none_keys}))}
    arrays.update({'state/' + k: v.numpy().astype(np.float16) for k, v in state.items()})
    arrays.update({'grad/' + k: v.numpy() for k, v in grads.items() if v is not None})
    arrays.update({'err/' + k: np.float64(v) for k, v in err.items()})
    np.savez(TH.FIXTURE, **arrays)
    print(f'{TH.FIXTURE}: max |out| {float(out.abs().max()):.3f}, None gradients {none_keys}, reference fp32 vs fp64: output {err_out:.2e}, '
          f'gradients {rel:.2e} of each tensor\'s max-abs; restatement within {worst:.2f} of its tolerances; {os.path.getsize(TH.FIXTURE)} bytes')


if __name__ == '__main__':
    main()
