"""The recorded spectral buffers of the HiFi-GAN scale discriminator's fixture state (tests/golden/hifigan_msd_spectral.npz,
tools/make_golden_hifigan_msd_spectral.py).

tests/hifigan_disc_helpers.fixture_inputs() regenerates the 30 M-float state from a seed.  Everything in it is element-wise and reproduces on any
host, except discriminator 0's weight_u / weight_v: they come out of float32 power iterations (matrix-vector sums, whose order of additions is the
host BLAS's) and are then rounded to float16, so a value next to a rounding tie lands on either side of it depending on the CPU - one float16 step,
1.5e-5 at 0.03, more than the 1e-5 the buffers are compared at.  The 16 buffers (18.5 k floats) are therefore data: recorded once on the host
whose regeneration equals the reference fixture's own recording of weight_u bit for bit, and laid over the regenerated state here."""
import os

import numpy as np
import torch

from tests import hifigan_disc_helpers as DH

SPECTRAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hifigan_msd_spectral.npz')


def spectral_keys():
    return [p + n for p in DH.prefixes(0) for n in ('weight_u', 'weight_v')]


def recorded_spectral():
    z = np.load(SPECTRAL)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def fixture_inputs():
    """DH.fixture_inputs() with discriminator 0's spectral buffers taken from the recording: (state, y, y_hat), the same on every host"""
    state, y, y_hat = DH.fixture_inputs()
    rec = recorded_spectral()
    assert sorted(rec) == sorted(spectral_keys())
    for k, v in rec.items():
        assert v.shape == state[k].shape and v.dtype == state[k].dtype, k
        state[k] = v.clone()
    return state, y, y_hat
