"""Developer tool (CPU): records tests/golden/hifigan_msd_spectral.npz - discriminator 0's 16 spectral buffers (weight_u, weight_v) of the state
tests/hifigan_disc_helpers.fixture_inputs() regenerates - on a host whose regeneration equals the reference fixture's own recording of weight_u
(tests/golden/hifigan_disc_ref.npz, eval/u0 .. eval/u7) bit for bit; refuses to write anything on a host where it does not.  Why the buffers are
data: tests/hifigan_msd_helpers.py.

    python tools/make_golden_hifigan_msd_spectral.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import hifigan_disc_helpers as DH
    from tests import hifigan_msd_helpers as SH
    state = DH.fixture_inputs()[0]
    fx = DH.fixture()
    for l, p in enumerate(DH.prefixes(0)):
        if not torch.equal(state[p + 'weight_u'], torch.from_numpy(fx[f'eval/u{l}'])):
            raise SystemExit(f'make_golden_hifigan_msd_spectral: this host regenerates {p}weight_u differently from the recorded fixture; nothing written')
    np.savez(SPECTRAL := SH.SPECTRAL, **{k: state[k].numpy() for k in SH.spectral_keys()})
    print(f'{SPECTRAL}: {len(SH.spectral_keys())} buffers, {sum(state[k].numel() for k in SH.spectral_keys())} floats, {os.path.getsize(SPECTRAL)} bytes')


if __name__ == '__main__':
    main()
