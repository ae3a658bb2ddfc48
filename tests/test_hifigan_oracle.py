"""Row f2 groundwork: the HiFi-GAN / NSF-HiFi-GAN generator oracle (oracle/hifigan_oracle.py) bit-for-bit against what the live reference
generator computed - with and without the NSF pitch source, before and after remove_weight_norm() - recorded in tests/golden/live_hifigan_*.npz
by oracle/make_golden_live.py (build container): the reference's parameter tree, the digests of its weights in both forms and its waveforms."""
import ast
import os

import pytest

from oracle.make_golden_live import digest, hifigan_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('resblock', ['1', '2'])
@pytest.mark.parametrize('nsf', [False, True])
def test_hifigan_oracle_bit_equal_to_live_reference(nsf, resblock):
    import numpy as np
    import torch
    from oracle import hifigan_oracle as HO
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', f'live_hifigan_{int(nsf)}_{resblock}.npz'))
    h = ast.literal_eval(str(ref['h']))
    assert h['use_pitch_embed'] == nsf and h['resblock'] == resblock
    mine, g = hifigan_params(h)                          # the HIP module's parameter tree == the reference module's; the weights it was given
    B, T = 2, 37
    mel = torch.randn(B, 80, T, generator=g)
    assert np.array_equal(mel.numpy(), ref['mel'])
    f0 = None
    if nsf:
        f0 = torch.rand(B, T, generator=g) * 300 + 80
        f0[0, 10:15] = 0
        f0[1, 30:] = 0
        assert np.array_equal(f0.numpy(), ref['f0'])
    for stage in ('weight_norm', 'plain'):
        if stage == 'plain':
            mine.remove_weight_norm()
        sd = mine.state_dict()
        want = {k: (s, d) for k, s, d in zip(ref[f'{stage}_keys'], ref[f'{stage}_shapes'], ref[f'{stage}_digests'])}
        assert {k: repr(tuple(v.shape)) for k, v in sd.items()} == {k: s for k, (s, _) in want.items()}, stage
        for k, v in sd.items():                          # the oracle gets the reference's weights bit for bit
            assert digest(v) == want[k][1], (stage, k)
        p = {k: v.detach().clone() for k, v in sd.items()}
        with torch.no_grad():
            torch.manual_seed(99)
            b = HO.generator(p, h, mel, f0)
        assert b.shape == (B, 1, T * 256), b.shape
        assert np.array_equal(b.numpy(), ref[f'{stage}_wav']), (stage, float(np.abs(b.numpy() - ref[f'{stage}_wav']).max()))


@pytest.mark.parametrize('name', ['hifigan_plain', 'hifigan_nsf'])
def test_hifigan_oracle_matches_reference_fixture_bitwise(name):
    """Everywhere (no reference needed): the oracle against the fixture oracle/make_golden_hifigan.py recorded from the reference."""
    import numpy as np
    import torch
    from oracle import hifigan_oracle as HO
    from oracle.make_golden_hifigan import CASES, CONFIG, inputs
    case = CASES[name]
    h = dict(CONFIG, use_pitch_embed=case['nsf'])
    p = HO.synth_generator_params(h, case['seed'] + 1000)
    mel, f0 = inputs(case)
    with torch.no_grad():
        torch.manual_seed(case['seed'])
        wav = HO.generator(p, h, mel, f0)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))['wav']
    assert wav.shape == g.shape == (case['B'], 1, case['T'] * 256)
    np.testing.assert_array_equal(wav.numpy(), g)
    assert 0.01 < float(np.abs(g).max()) <= 1.0
