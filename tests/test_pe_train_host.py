"""CPU: the ABI of the PitchExtractor training operators (declared, bound, exported; arguments rejected before any device call), the module's
refusal to run without the device in train mode, and the fixture recorded from the reference's own PitchExtractor().train()
(tools/make_golden_pe_train.py) against the float64 restatement of tests/pe_train_helpers.py."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import diffsinger_amd
from diffsinger_amd import _lib, hparams
from oracle import pe_oracle as PO
from tests import pe_train_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['dsf_batch_norm_train', 'dsf_batch_norm_train_bwd', 'dsf_group_norm_bwd_workspace_floats', 'dsf_group_norm_bwd',
       'dsf_f0_loss_workspace_floats', 'dsf_f0_loss', 'dsf_f0_loss_bwd']
P = 64                      # a non-null "pointer": the argument checks never dereference it


def test_new_symbols_declared_bound_and_exported():
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dsf.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.lib_path())
    lib = _lib.load()
    for name in NEW:
        assert re.search(r'\b(int|int64_t)\s+%s\s*\(' % name, code), name
        assert name in _lib.SYMBOLS_FS2, name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert 'pe_train.hpp' in open(os.path.join(ROOT, 'diffsinger_amd', 'csrc', 'dsd.hip')).read()
    from diffsinger_amd import build
    assert os.path.join(ROOT, 'diffsinger_amd', 'csrc', 'pe_train.hpp') in build.DEPS
    for name in ('pe_losses', 'pe_training_step'):
        assert name in diffsinger_amd.__all__ and callable(getattr(diffsinger_amd, name))
    assert lib.dsf_group_norm_bwd_workspace_floats(3, 64) == 3 * 2 * 64
    assert lib.dsf_group_norm_bwd_workspace_floats(0, 64) == -1
    assert lib.dsf_f0_loss_workspace_floats() >= 4


def test_bad_arguments_are_rejected_without_a_device():
    lib = _lib.load()
    bn = lambda *a: lib.dsf_batch_norm_train(*a)
    assert bn(None, P, P, None, P, P, P, None, None, 2, 8, 4, 1e-5, 0.1, 1, None) == -1
    assert b'dsf_batch_norm_train' in lib.dsd_last_error()
    assert bn(P, P, P, None, None, P, P, None, None, 2, 8, 4, 1e-5, 0.1, 1, None) == -1
    assert bn(P, P, P, None, P, P, P, None, None, 1, 8, 1, 1e-5, 0.1, 1, None) == -1            # B * T < 2: torch raises there too
    assert b'more than one value' in lib.dsd_last_error()
    assert bn(P, P, P, None, P, P, P, None, None, 0, 8, 4, 1e-5, 0.1, 1, None) == -1
    bw = lambda *a: lib.dsf_batch_norm_train_bwd(*a)
    assert bw(P, P, P, P, None, None, P, P, P, 2, 8, 4, 1, None) == -1
    assert bw(P, P, P, P, P, None, P, P, P, 1, 8, 1, 1, None) == -1
    assert b'dsf_batch_norm_train_bwd' in lib.dsd_last_error()
    gn = lambda *a: lib.dsf_group_norm_bwd(*a)
    assert gn(P, P, P, None, P, P, P, P, 2, 64, 4, 8, 1e-5, 1, None) == -1
    assert gn(P, P, P, P, P, P, P, None, 2, 64, 4, 8, 1e-5, 1, None) == -1
    assert gn(P, P, P, P, P, P, P, P, 2, 64, 5, 8, 1e-5, 1, None) == -1                         # groups must divide C
    assert b'dsf_group_norm_bwd' in lib.dsd_last_error()
    assert lib.dsf_f0_loss(None, 2, 2, 1, P, P, P, 2, 8, 2, 1, 0, 1.0, 1.0, P, P, None) == -1
    assert lib.dsf_f0_loss(P, 2, 2, 1, P, None, P, 2, 8, 2, 1, 0, 1.0, 1.0, P, P, None) == -1    # use_uv without uv
    assert lib.dsf_f0_loss(P, 2, 2, 1, P, P, P, 2, 8, 1, 1, 0, 1.0, 1.0, P, P, None) == -1       # use_uv needs two channels
    assert b'dsf_f0_loss' in lib.dsd_last_error()
    assert lib.dsf_f0_loss_bwd(P, 2, 2, 1, P, P, P, 2, 8, 2, 1, 0, 1.0, 1.0, None, P, P, None) == -1
    assert lib.dsf_f0_loss_bwd(P, 2, 2, 1, P, P, P, 2, 0, 2, 1, 0, 1.0, 1.0, P, P, P, None) == -1
    assert b'dsf_f0_loss_bwd' in lib.dsd_last_error()
    # LayerNorm widths: a multiple of 8 up to 256
    assert lib.dsf_layer_norm(P, P, P, P, 1, 60, 4, 1e-5, 0, None, None) == -1
    assert lib.dsf_layer_norm(P, P, P, P, 1, 264, 4, 1e-5, 0, None, None) == -1


def _module(train=True):
    hparams.clear()
    hparams.update(PH.HP, dur_loss='mse')
    from diffsinger_amd.pe import PitchExtractor
    m = PitchExtractor()
    return m.train() if train else m.eval()


def test_train_mode_has_no_cpu_path():
    m = _module()
    with pytest.raises(RuntimeError, match='no CPU path'):
        m(torch.zeros(1, 8, 80))
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.mel_prenet(torch.zeros(1, 8, 80))
    from diffsinger_amd.pe import pe_losses, pe_training_step
    with pytest.raises(RuntimeError, match='no CPU path'):
        pe_training_step(m, {'mels': torch.zeros(1, 8, 80), 'f0': torch.zeros(1, 8), 'uv': torch.zeros(1, 8)}, PH.HP)
    with pytest.raises(NotImplementedError):
        pe_losses({'pitch_pred': torch.zeros(1, 8, 2)}, {'mels': torch.zeros(1, 8, 80), 'f0': torch.zeros(1, 8), 'uv': torch.zeros(1, 8)},
                  dict(PH.HP, pitch_loss='ssim'))
    m.mel_prenet.layers[0][2].momentum = None
    from diffsinger_amd.pe import batch_norm_train_cm
    with pytest.raises(NotImplementedError, match='momentum'):
        batch_norm_train_cm(torch.zeros(1, 64, 32), 8, m.mel_prenet.layers[0][2])


def _fixture():
    return np.load(PH.FIXTURE)


def test_fixture_is_complete():
    g = _fixture()
    hp = ast.literal_eval(str(g['hp']))
    assert hp == PH.HP and int(g['seed']) == PH.CASE['seed'] and (int(g['B']), int(g['T'])) == (PH.CASE['B'], PH.CASE['T'])
    assert float(g['relu_min_ratio']) >= PH.RELU_MARGIN
    m = _module()
    params = dict(m.named_parameters())
    assert set(params) == {k for k in PO.extractor_shapes(hp) if PH.is_param(k)}
    keys = ['pitch_pred', 'loss/uv', 'loss/f0'] + ['grad/' + k for k in params]
    for l in range(3):
        keys += [f'running/mel_prenet.layers.{l}.2.running_mean', f'running/mel_prenet.layers.{l}.2.running_var']
        assert int(g[f'running/mel_prenet.layers.{l}.2.num_batches_tracked']) == 8
    for k in keys:
        assert k in g.files and 'dev/' + k in g.files, k
        assert np.isfinite(g[k]).all() and 0 <= float(g['dev/' + k]) < 1e-4, k
    for k, v in params.items():
        assert g['grad/' + k].shape == tuple(v.shape) and np.abs(g['grad/' + k]).max() > 0, k
    assert g['pitch_pred'].shape == (PH.CASE['B'], PH.CASE['T'], 2)
    assert os.path.getsize(PH.FIXTURE) < (1 << 20)


def test_float64_restatement_reproduces_the_fixture():
    g = _fixture()
    state, mel, f0, uv = PH.case_inputs()
    want = PH.training_step(state, PH.HP, mel, f0, uv, torch.float64)
    got = {'pitch_pred': want['pitch_pred'], 'loss/uv': want['uv'], 'loss/f0': want['f0']}
    got.update({'grad/' + k: v for k, v in want['grad'].items()})
    got.update({'running/' + k: v for k, v in want['running'].items() if not k.endswith('num_batches_tracked')})
    assert len(got) == len([k for k in g.files if k.startswith('dev/')])
    for k, v64 in got.items():
        err, dev = PH.rel_err(torch.from_numpy(np.asarray(g[k])), v64), float(g['dev/' + k])
        assert err <= dev * 1.001 + 1e-12, (k, err, dev)           # the recorded fp32 deviation (a float64 sum may round differently on another host)
    # and the fp32 run of the same restatement is a valid "second correct fp32 evaluation": no ReLU input changes sign
    r32 = PH.training_step(state, PH.HP, mel, f0, uv, torch.float32)
    ratio, flips = PH.relu_condition(r32['relu'], want['relu'])
    assert flips == 0 and ratio >= PH.RELU_MARGIN, (ratio, flips)
