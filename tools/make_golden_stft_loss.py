"""Developer tool (CPU, needs the reference checkout): writes tests/golden/stft_loss_ref.npz from the REFERENCE'S OWN module code.

    python tools/make_golden_stft_loss.py [--reference /path/to/reference]        (default: $DIFFSINGER_REFERENCE, oracle/ref_driver.py's rule)

modules/parallel_wavegan/losses/stft_loss.py is loaded by file path and its MultiResolutionSTFTLoss() runs with its defaults (the three
resolutions of configs/tts/pwg.yaml:77-82) in float32 on the CPU.  The module calls torch.stft without return_complex, which torch 2.x
refuses: for the duration of the call torch.stft is wrapped to pass return_complex=True and hand back view_as_real - the (..., 2) layout
the module indexes.  Nothing else is replaced.

Stored: x, y (1 x 8000 float32: the 'near' pair of tests/stft_loss_helpers.py, first row), sc, mag (float32) and d sc / dx, d mag / dx."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import stft_loss_helpers as LH  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'stft_loss_ref.npz')


def load_reference_module(root):
    path = os.path.join(root, 'modules', 'parallel_wavegan', 'losses', 'stft_loss.py')
    spec = importlib.util.spec_from_file_location('reference_stft_loss', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class complex_stft:
    """torch.stft(..., return_complex=True) handed back as view_as_real while the block runs"""

    def __enter__(self):
        self.orig = orig = torch.stft
        torch.stft = lambda *a, **k: torch.view_as_real(orig(*a, return_complex=True, **k))

    def __exit__(self, *exc):
        torch.stft = self.orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DIFFSINGER_REFERENCE', '/root/reference'))
    args = ap.parse_args()
    crit = load_reference_module(args.reference).MultiResolutionSTFTLoss()
    x, y = LH.signals('near')
    x, y = x[:1].clone(), y[:1].clone()
    xg = x.clone().requires_grad_(True)
    with complex_stft():
        sc, mag = crit(xg, y)
        g_sc, = torch.autograd.grad(sc, xg, retain_graph=True)
        g_mag, = torch.autograd.grad(mag, xg)
    assert sc.dtype == mag.dtype == torch.float32
    sc, mag = sc.detach(), mag.detach()
    np.savez(OUT, x=x.numpy(), y=y.numpy(), sc=sc.numpy(), mag=mag.numpy(), g_sc=g_sc.numpy(), g_mag=g_mag.numpy())
    print(f'{OUT}: sc {float(sc):.8f} mag {float(mag):.8f}, max |d sc/dx| {float(g_sc.abs().max()):.3e}, max |d mag/dx| {float(g_mag.abs().max()):.3e}, '
          f'{os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
