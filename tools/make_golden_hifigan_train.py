"""Developer tool (CPU, needs the reference checkout): writes tests/golden/hifigan_train_ref.npz from the REFERENCE'S OWN module code.

    python tools/make_golden_hifigan_train.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE)

modules.hifigan.hifigan.HifiGanGenerator is imported from the reference tree as tools/make_golden_pwg_train.py imports its module (scipy.signal.kaiser
aliased, librosa / pycwt stubbed).  Nothing of the reference's program text is copied; the fixture holds data only.  Configuration:
tests/hifigan_train_helpers.FIXTURE_CFG (resblock '1', rates [4, 4, 2, 2], initial channel 32, weight norm on: 66.7 k parameters), B = 1, T = 8 frames.
Two cases, each under its own prefix:

  plain/   use_pitch_embed off
  nsf/     use_pitch_embed on, f0 with an unvoiced stretch, the source module's draws by torch.manual_seed(seed) (tests/voc_helpers.
           draws_like_reference(seed, ...) reproduces them)

  * 'state': the seeded O(1) state of hifigan_train_helpers.synth_state rounded to float16 (stored as float16 without loss), every tensor
    flattened and concatenated in the order of 'keys' / 'shapes' of 'meta_json' (one array: an npz entry per tensor costs more than the data);
  * 'x' mel, 'f0', 'target'; the module's float32 CPU output 'out' and every parameter gradient under L = mean((y - target)^2) in 'grads',
    concatenated alike (keys without a gradient left out);
  * 'masks': x > 0 of every leaky-ReLU input of the float32 run in call order, bit-packed ('meta_json' holds their shapes, the configuration, the
    seed and the keys whose gradient autograd leaves at None); for nsf 'sine_waves' [B][L][9], the output of the module's SineGen;
  * 'err' = max|grad_fp32 - grad_fp64| per gradient key and 'err_out' of the reference module itself (its .double() copy, fed the float32 run's sine_waves).

A seed for which the module's float32 and float64 runs disagree on any leaky-ReLU mask is refused (one flipped sign moves whole gradient tensors
by thousands of times the rule) and the next one is tried; the seed used is printed and recorded.  Before anything is written the float64
restatement of tests/hifigan_train_helpers.py on the recorded masks must reproduce the recorded gradients within the test's own tolerances."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hifigan_train_helpers as TH  # noqa: E402

FIRST_SEED, B, FRAMES = 20240701, 1, 8


def reference_class(root):
    sys.dont_write_bytecode = True
    for n in ('librosa', 'pycwt'):
        sys.modules.setdefault(n, types.ModuleType(n))
    import scipy.signal
    import scipy.signal.windows
    if not hasattr(scipy.signal, 'kaiser'):
        scipy.signal.kaiser = scipy.signal.windows.kaiser
    sys.path.insert(0, root)
    from modules.hifigan.hifigan import HifiGanGenerator
    return HifiGanGenerator


class Recorder:
    """records the input of every F.leaky_relu call while active (the reference calls it through torch.nn.functional)"""

    def __enter__(self):
        import torch.nn.functional as F
        self.F, self.orig, self.pre = F, F.leaky_relu, []

        def wrapped(x, *a, **k):
            self.pre.append(x.detach())
            return self.orig(x, *a, **k)
        F.leaky_relu = wrapped
        return self

    def __exit__(self, *exc):
        self.F.leaky_relu = self.orig


def run(module, x, f0, target, seed, sine_waves=None):
    """-> (out, grads, masks, sine_waves of the module's SineGen)"""
    module.zero_grad()
    got, hooks = {}, []
    if f0 is not None:
        def hook(mod, inp, out):
            got['sw'] = out[0].detach()
            if sine_waves is not None:
                return (sine_waves.to(out[0].dtype),) + tuple(out[1:])
        hooks.append(module.m_source.l_sin_gen.register_forward_hook(hook))
    torch.manual_seed(seed)
    with Recorder() as rec:
        y = module(x, f0) if f0 is not None else module(x)
    for hk in hooks:
        hk.remove()
    torch.mean((y - target) ** 2).backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in module.named_parameters()}
    return y.detach(), grads, TH.masks_of(rec.pre), got.get('sw')


def make_case(Ref, nsf, seed):
    h = TH.config(use_pitch_embed=nsf)
    m = Ref(h)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == TH.module_shapes(h), set(shapes) ^ set(TH.module_shapes(h))
    state = {k: v.half().float() for k, v in TH.synth_state(shapes, seed).items()}
    m.load_state_dict(state, strict=True)
    hop = TH.hop_of(h)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 80, FRAMES, generator=gen)
    target = 0.5 * torch.randn(B, 1, FRAMES * hop, generator=gen)
    f0 = None
    if nsf:
        f0 = 180.0 + 60.0 * torch.rand(B, FRAMES, generator=gen)
        f0[:, 3:5] = 0.0                                                    # an unvoiced stretch
    out, grads, masks, sw = run(m, x, f0, target, seed)
    m64 = Ref(h)
    m64.load_state_dict(state, strict=True)
    m64 = m64.double()
    out64, grads64, masks64, _ = run(m64, x.double(), None if f0 is None else f0.double(), target.double(), seed, sine_waves=sw)
    flips, n = TH.count_flips(masks, masks64)
    if flips:
        return None, f'seed {seed}: {flips} of {n} leaky-ReLU inputs change sign between the module\'s float32 and float64 runs'
    none_keys = sorted(k for k, g in grads.items() if g is None)
    assert none_keys == sorted(k for k, g in grads64.items() if g is None)
    err = {k: float((grads[k].double() - grads64[k]).abs().max()) for k in grads if grads[k] is not None}
    err_out = float((out.double() - out64).abs().max())
    # the helper: bitwise the module in float32 (same draws), and its float64 on the recorded masks within the test's tolerances
    torch.manual_seed(seed)
    o32, _, _, pre32, sw32 = TH.module_grads(state, h, x, f0, TH.mse_to(target), dtype=torch.float32)
    assert torch.equal(o32, out), 'the float32 restatement is not bitwise the reference module'
    assert TH.count_flips(TH.masks_of(pre32), masks)[0] == 0 and (sw is None or torch.equal(sw32, sw))
    o_h, g_h, dw_h, _, _ = TH.module_grads(state, h, x, f0, TH.mse_to(target), masks=masks, sine_waves=sw)
    assert sorted(k for k, g in g_h.items() if g is None) == none_keys, 'the restatement leaves other gradients at None'
    assert float((o_h - out.double()).abs().max()) <= max(4 * err_out, TH.RULE * float(o_h.abs().max()))
    tol = TH.tolerances(state, g_h, dw_h, err)
    worst = 0.0
    for k, t in tol.items():
        e = float((grads[k].double() - g_h[k]).abs().max())
        assert e <= t, f'{k}: the float64 restatement misses the reference by {e:.3e} (tolerance {t:.3e})'
        worst = max(worst, e / t)
    keys = sorted(state)
    gkeys = [k for k in keys if grads[k] is not None]
    flat = lambda d, ks, dt: np.concatenate([d[k].numpy().reshape(-1) for k in ks]).astype(dt)                   # noqa: E731
    arrays = {'x': x.numpy(), 'target': target.numpy(), 'out': out.numpy(), 'err_out': np.float64(err_out), 'masks': TH.pack_masks(masks),
              'state': flat(state, keys, np.float16), 'grads': flat(grads, gkeys, np.float32), 'err': np.array([err[k] for k in gkeys], np.float64),
              'meta_json': np.array(json.dumps({'h': h, 'none_keys': none_keys, 'seed': seed, 'mask_shapes': [list(mk.shape) for mk in masks],
                                                'keys': keys, 'shapes': [list(state[k].shape) for k in keys]}))}
    if nsf:
        arrays.update({'f0': f0.numpy(), 'sine_waves': sw.numpy()})
    info = (f'seed {seed}, {n} leaky-ReLU inputs, max |out| {float(out.abs().max()):.3f}, None gradients {none_keys}, reference fp32 vs fp64: output '
            f'{err_out:.2e}; restatement within {worst:.2f} of its tolerances')
    return arrays, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE'))
    args = ap.parse_args()
    if not args.reference:
        raise SystemExit('make_golden_hifigan_train: pass --reference or set DIFFSINGER_REFERENCE to the reference checkout')
    Ref = reference_class(args.reference)
    out = {}
    for case in TH.CASES:
        for seed in range(FIRST_SEED, FIRST_SEED + 16):
            arrays, info = make_case(Ref, case == 'nsf', seed)
            if arrays is not None:
                break
            print(f'{case}: refused - {info}')
        else:
            raise SystemExit(f'{case}: no seed in [{FIRST_SEED}, {FIRST_SEED + 16}) keeps the float32 and float64 masks equal')
        print(f'{case}: {info}')
        out.update({f'{case}/{k}': v for k, v in arrays.items()})
    np.savez_compressed(TH.FIXTURE, **out)
    size = os.path.getsize(TH.FIXTURE)
    assert size < (1 << 20), size
    print(f'{TH.FIXTURE}: {size} bytes')


if __name__ == '__main__':
    main()
