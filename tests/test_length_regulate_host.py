"""CPU: the host side of the length regulator on a frame budget (include/dsf.h dsf_length_regulate, fs2.FastSpeech2.forward(max_frames=)):
the restatement tests/regulate_helpers.py pinned to the recorded reference results, the ABI, the argument validation that runs before
any device work, and the refusals of the C entry point (argument checks come before the launch: no device needed)."""
import ctypes
import os
import re

import pytest
import torch

from diffsinger_amd import _lib
from oracle.fs2_cases import CASES, make_inputs
from tests import fs2_helpers as FH
from tests import regulate_helpers as RH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREE = ['fs2_lj_free', 'fs2_popcs_free', 'fs2_midi_e2e_free', 'fs2_lj_spkid_energy_free', 'fs2_popcs_ph_free']


@pytest.mark.parametrize('name', FREE)
def test_restatement_reproduces_the_recorded_reference_mel2ph(name):
    g = FH.load_golden(name)
    tok = make_inputs(CASES[name], False)['txt_tokens']
    logdur = torch.from_numpy(g['dur'][..., 0])
    choice, mel2ph, mel_len = RH.regulate(logdur=logdur, padding=(tok == 0))
    want = torch.from_numpy(g['mel2ph'])
    assert mel2ph.shape == want.shape and torch.equal(mel2ph, want)
    assert torch.equal(mel_len, (want > 0).sum(-1))
    assert torch.equal(choice, RH.out2dur64(logdur))                    # no token of the fixtures sits near a rounding boundary
    assert float(RH.half_distance64(logdur).min()) > 1e-3


def test_restatement_branches_are_exercised_by_the_fixtures():
    zeros = pads = 0
    for name in FREE:
        g = FH.load_golden(name)
        tok = make_inputs(CASES[name], False)['txt_tokens']
        d = RH.out2dur64(torch.from_numpy(g['dur'][..., 0]))
        zeros += int(((d == 0) & (tok != 0)).sum())
        pads += int((tok == 0).sum())
    assert zeros > 0 and pads > 0


def test_restatement_equals_the_mask_and_sum_formulation():
    """The upper-bound search against the reference's formulation (a [B, T_txt, T_mel] mask summed over tokens), on zero durations, padding
    and alpha != 1 - integer for integer."""
    g = torch.Generator().manual_seed(5)
    for i in range(60):
        B, Tt = int(torch.randint(1, 5, (1,), generator=g)), int(torch.randint(1, 40, (1,), generator=g))
        dur = torch.randint(0, 12, (B, Tt), generator=g) * (torch.rand(B, Tt, generator=g) > 0.3)
        pad = torch.rand(B, Tt, generator=g) > 0.8
        alpha = (0.8, 1.0, 1.3)[i % 3]
        d = torch.round(dur.float() * alpha).long() * (1 - pad.long())
        cs = torch.cumsum(d, 1)
        prev = cs - d
        pos = torch.arange(int(d.sum(-1).max()))[None, None]
        mask = (pos >= prev[:, :, None]) & (pos < cs[:, :, None])
        want = (torch.arange(1, Tt + 1)[None, :, None] * mask.long()).sum(1)
        _, got, mel_len = RH.regulate(dur=dur, padding=pad, alpha=alpha)
        assert torch.equal(got, want) and torch.equal(mel_len, d.sum(-1))


def test_length_regulate_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'dsf.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'\bint\s+dsf_length_regulate\s*\(', code)
    assert 'dsf_length_regulate' in _lib.SYMBOLS_FS2
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.lib_path()), 'dsf_length_regulate')
    assert lib.dsd_abi_version() == 8 and _lib.DSD_ABI_VERSION == 8
    abi = re.search(r'#define\s+DSD_ABI_VERSION\s+(\d+)', open(os.path.join(ROOT, 'include', 'dsd.h')).read())
    assert int(abi.group(1)) == 8
    assert int(re.search(r'#define\s+DSF_REGULATE_MAX_TXT\s+(\d+)', code).group(1)) == 4096


@pytest.mark.parametrize('name', ['fs2_lj_free', 'fs2_midi_e2e_free'])
def test_max_frames_is_validated_on_the_host(name):
    """A CPU-built module: the checks run before any device call (a device call on CPU tensors would raise RuntimeError, not ValueError)."""
    case, m, hp, params, inp = FH.case_setup(name)
    kw = {k: v for k, v in inp.items() if k != 'txt_tokens'}
    tok = inp['txt_tokens']
    for bad in (0, -3, 2.5, True, '7'):
        with pytest.raises(ValueError, match='max_frames'):
            m(tok, infer=True, max_frames=bad, **kw)
    with pytest.raises(ValueError, match='mel2ph'):
        m(tok, mel2ph=torch.ones(tok.shape[0], 9, dtype=torch.long), infer=True, max_frames=9, **kw)
    from diffsinger_amd import fs2
    with pytest.raises(ValueError, match='max_frames'):
        fs2.LengthRegulator()(torch.ones(1, 3, dtype=torch.long), max_frames=0)


def test_cpu_regulator_with_a_budget_equals_the_restatement():
    """LengthRegulator's torch sequence (CPU tensors) with max_frames: the rows cut or padded, no other change."""
    from diffsinger_amd import fs2
    g = torch.Generator().manual_seed(2)
    dur = torch.randint(0, 9, (3, 11), generator=g)
    pad = torch.zeros(3, 11, dtype=torch.bool)
    pad[1, 7:] = True
    reg = fs2.LengthRegulator()
    full = reg(dur, pad)
    for N in (5, full.shape[1], full.shape[1] + 13):
        _, want, _ = RH.regulate(dur=dur, padding=pad, T_out=N)
        assert torch.equal(reg(dur, pad, max_frames=N), want)
        assert torch.equal(want, RH.pad_frames(full, N))


def test_c_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                           # a non-NULL pointer that is never dereferenced: every call below is refused
    f = lib.dsf_length_regulate
    cases = {
        'neither dur nor logdur': (None, None, 1.0, None, 1.0, None, one, one, 1, 4, 8),
        'both dur and logdur': (one, one, 1.0, None, 1.0, None, one, one, 1, 4, 8),
        'alpha 0': (one, None, 1.0, None, 0.0, None, one, one, 1, 4, 8),
        'alpha negative': (one, None, 1.0, None, -1.0, None, one, one, 1, 4, 8),
        'alpha nan': (one, None, 1.0, None, float('nan'), None, one, one, 1, 4, 8),
        'B 0': (one, None, 1.0, None, 1.0, None, one, one, 0, 4, 8),
        'T_txt 0': (one, None, 1.0, None, 1.0, None, one, one, 1, 0, 8),
        'T_out 0': (one, None, 1.0, None, 1.0, None, one, one, 1, 4, 0),
        'T_txt above the maximum': (None, one, 1.0, None, 1.0, None, one, one, 1, 4097, 8),
        'no output': (one, None, 1.0, None, 1.0, None, None, None, 1, 4, 8),
    }
    for what, a in cases.items():
        assert f(*a, None) == -1, what
        assert b'dsf_length_regulate' in lib.dsd_last_error(), what
    f(None, one, 1.0, None, 1.0, None, one, one, 1, 4097, 8, None)
    assert b'4096' in lib.dsd_last_error()
