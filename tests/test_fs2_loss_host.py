"""CPU: the host side of the FastSpeech2 objective (diffsinger_amd/losses.py) - mel_loss parsing, the word segmentation maths the duration
kernels implement, the Gaussian window baked into csrc/fs2_loss.hpp, and the restatement tests/fs2_loss_helpers.py against the reference's
own code where that imports (modules/commons/ssim.py, mel2ph_to_dur; skipped without the reference tree)."""
import importlib.util
import os
import re

import pytest
import torch

from diffsinger_amd import losses
from oracle.ref_driver import REFERENCE_ROOT, reference_available
from tests import fs2_loss_helpers as LH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mel_loss_parsing_follows_the_task():
    assert losses.parse_mel_loss('l1') == {'l1': 1.0}
    assert losses.parse_mel_loss('ssim:0.5|l1:0.5') == {'ssim': 0.5, 'l1': 0.5}
    assert list(losses.parse_mel_loss('ssim:0.5|l1:0.5')) == ['ssim', 'l1']         # the dict's key order is the config's
    assert losses.parse_mel_loss('l1:0.5|ssim:0.5|') == {'l1': 0.5, 'ssim': 0.5}
    assert losses.parse_mel_loss('') == {}


def test_sil_phone_ids():
    assert losses.sil_phone_ids(['<pad>', '<EOS>', '<UNK>', 'a', 'SP', ',', 'b1', '|']) == [0, 1, 2, 5, 7]


def _segments_like_the_kernel(tok, sil=None, wdb=None):
    """The slot of every phone as k_dur_loss_rows assigns it: (a) cumsum(is_sil) - 1 for non-silence phones (word 0 dropped, -1 = none),
    (b) the exclusive prefix sum of word_boundary."""
    if wdb is None:
        is_sil = torch.isin(tok, torch.tensor(sil))
        cs = is_sil.long().cumsum(-1)
        return torch.where(is_sil, torch.full_like(cs, -1), cs - 1)
    return wdb.cumsum(-1) - wdb


def test_word_segmentation_index_maths():
    tok = torch.tensor([[3, 1, 4, 4, 2, 5, 0, 0], [4, 4, 4, 4, 4, 4, 4, 4], [1, 4, 1, 1, 5, 6, 2, 0]])
    sil = [0, 1, 2]
    slots = _segments_like_the_kernel(tok, sil=sil)
    is_sil = torch.isin(tok, torch.tensor(sil)).float()
    word_id = (is_sil.cumsum(-1) * (1 - is_sil)).long()                              # tasks/tts/fs2.py:208
    assert torch.equal(torch.where(word_id > 0, word_id - 1, torch.full_like(word_id, -1)), slots)
    assert int(slots.max()) < tok.shape[1]                                            # the word buffer of T_txt slots suffices
    wdb = torch.tensor([[0, 1, 0, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0]])
    idx = torch.nn.functional.pad(wdb.cumsum(axis=1), (1, 0))[:, :-1]                 # usr/diffsinger_task.py:377
    assert torch.equal(idx, _segments_like_the_kernel(tok, wdb=wdb))
    for row in idx:                                                                   # words are contiguous runs (summed in phone order)
        assert bool((row[1:] >= row[:-1]).all())


def test_window_constants_are_the_reference_fp32_values():
    src = open(os.path.join(ROOT, 'diffsinger_amd', 'csrc', 'fs2_loss.hpp')).read()
    body = re.search(r'kSsimG\[11\]\s*=\s*\{([^}]*)\}', src).group(1)
    vals = [float.fromhex(v.strip().rstrip('f')) for v in body.split(',')]
    assert vals == [float(v) for v in LH.gaussian(11, 1.5)]


def _ref_module(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE_ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not reference_available(), reason='reference tree not mounted')
def test_restated_ssim_matches_the_reference_module():
    S = _ref_module('modules/commons/ssim.py', 'ref_ssim')
    assert torch.equal(S.gaussian(11, 1.5), LH.gaussian(11, 1.5))
    assert torch.equal(S.create_window(11, 1), LH.create_window(11))
    x, y = LH.mel_case(2, 40, 80, seed=1)
    a, b = x[:, None] + 6.0, y[:, None] + 6.0
    for dt in (torch.float32, torch.float64):
        w = S.create_window(11, 1).to(dt)                                             # fp64: create_window + _ssim (the module caches its window)
        want = S._ssim(a.to(dt), b.to(dt), w, 11, 1, size_average=False)
        got = LH.ssim_map(a.to(dt), b.to(dt)).mean(1)
        assert torch.equal(got, want)
    w = S.create_window(11, 1)
    ref_loss = 1 - S._ssim(a, b, w, 11, 1, size_average=False)
    wt = LH.weights_nonzero_speech(y)
    assert torch.equal((ref_loss * wt).sum() / wt.sum(), LH.ssim_loss(x, y))


@pytest.mark.skipif(not reference_available(), reason='reference tree not mounted')
def test_restated_mel2ph_to_dur_matches_the_reference():
    import sys
    sys.path.insert(0, REFERENCE_ROOT)
    try:
        from modules.fastspeech.tts_modules import mel2ph_to_dur
    except Exception as e:                                                            # pragma: no cover - depends on the reference's imports
        pytest.skip(f'modules.fastspeech.tts_modules does not import here: {e}')
    finally:
        sys.path.remove(REFERENCE_ROOT)
    g = torch.Generator().manual_seed(4)
    mel2ph = torch.randint(0, 13, (3, 50), generator=g)
    assert torch.equal(mel2ph_to_dur(mel2ph, 12), LH.mel2ph_to_dur(mel2ph, 12))


def test_restated_duration_loss_of_a_hand_case():
    """pdur / wdur / sdur of one utterance worked out by hand from tasks/tts/fs2.py:190-219 (silence ids) and the MIDI form (word_boundary)."""
    import math
    tok = torch.tensor([[1, 5, 6, 1, 7, 0]])
    mel2ph = torch.tensor([[1, 2, 2, 3, 5, 5, 5, 0]])                                 # phone 4 gets no frame, phone 6 is padding
    dp = torch.tensor([[0.1, 0.7, 0.2, -0.3, 1.1, 0.4]], dtype=torch.float64)
    L = LH.dur_loss(dp, mel2ph, tok, sil_ids=[1], lam_ph=1.0, lam_word=1.0, lam_sent=1.0)
    g = [1, 2, 1, 0, 3, 0]
    npd = [1, 1, 1, 1, 1, 0]
    pd = sum((float(dp[0, i]) - math.log(g[i] + 1)) ** 2 * npd[i] for i in range(6)) / 5
    lin = [max(math.exp(float(v)) - 1, 0) for v in dp[0]]
    words = [(lin[1] + lin[2], 3.0), (lin[4] + lin[5], 3.0)]                          # word 0 (phone 0 and the silences) dropped; id 0 is no silence here
    wd = sum((math.log(p + 1) - math.log(q + 1)) ** 2 for p, q in words) / 2
    sd = (math.log(sum(lin) + 1) - math.log(sum(g) + 1)) ** 2
    assert abs(float(L['pdur']) - pd) < 1e-12 and abs(float(L['wdur']) - wd) < 1e-12 and abs(float(L['sdur']) - sd) < 1e-12


def test_cpu_tensors_are_refused():
    with pytest.raises(ValueError):
        losses.mel_loss_terms(torch.zeros(1, 5, 80), torch.zeros(1, 5, 80))
    with pytest.raises(ValueError):
        losses.dur_loss_terms(torch.zeros(1, 4), torch.zeros(1, 6, dtype=torch.long), torch.ones(1, 4, dtype=torch.long), sil_ids=[1])
    with pytest.raises(ValueError):
        losses.ssim(torch.zeros(1, 1, 5, 80), torch.zeros(1, 1, 5, 80), window_size=9)
    with pytest.raises(NotImplementedError):
        losses.fs2_losses({}, {'mels': None, 'txt_tokens': None, 'mel2ph': None}, {'dur_loss': 'mog'})
