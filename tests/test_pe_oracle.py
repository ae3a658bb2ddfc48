"""Row f2: the PitchExtractor oracle (oracle/pe_oracle.py) against the reference-generated fixture and bit-for-bit against what the live
reference module computed on a second input (tests/golden/live_pe.npz, recorded by oracle/make_golden_live.py in the build container)."""
import ast
import os

import numpy as np
import torch

from oracle import pe_oracle as PO
from oracle.make_golden_pe import CASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'pe_opencpop.npz'))
    return g, ast.literal_eval(str(g['hp']))


def test_pe_oracle_matches_reference_fixture_bitwise():
    g, hp = golden()
    p = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in PO.synth_extractor_params(hp, CASE['seed'] + 1000).items()}
    mel = PO.synth_mel(CASE['B'], CASE['T'], CASE['seed'])
    with torch.no_grad():
        r = PO.pitch_extractor(p, hp, mel)
    np.testing.assert_array_equal(r['pitch_pred'].numpy(), g['pitch_pred'])
    np.testing.assert_array_equal(r['f0_denorm_pred'].numpy(), g['f0_denorm_pred'])
    f0 = g['f0_denorm_pred']
    assert (f0[1, -5:] == 0).all() and (f0[2, -10:] == 0).all()            # padding frames
    assert 0.2 < (f0 > 0).mean() < 0.9 and f0.max() < 2000                  # voiced and unvoiced frames both present


def test_pe_oracle_bit_equal_to_live_reference():
    from oracle.make_golden_live import digest
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'live_pe.npz'))
    hp = ast.literal_eval(str(ref['hp']))
    p = PO.synth_extractor_params(hp, 4242)
    assert sorted(p) == sorted(ref['state_dict_keys'])
    for k, d in zip(ref['state_dict_keys'], ref['state_dict_digests']):     # the weights the reference module held, bit for bit
        assert digest(p[k]) == d, k
    mel = PO.synth_mel(2, 83, 77)
    with torch.no_grad():
        b = PO.pitch_extractor(p, hp, mel)
    for k in ('pitch_pred', 'f0_denorm_pred'):
        assert np.array_equal(b[k].numpy(), ref[k]), (k, float(np.abs(b[k].numpy() - ref[k]).max()))
