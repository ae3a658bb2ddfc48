"""GPU: the length regulator as one HIP operator (include/dsf.h dsf_length_regulate) and the free-running FastSpeech2 forward on a frame
budget (fs2.FastSpeech2.forward(max_frames=N)): no host read, capturable, the same computation as a teacher-forced call with the padded
mel2ph.  Integer results are compared with torch.equal against the CPU restatement tests/regulate_helpers.py (pinned to the recorded
reference results by tests/test_length_regulate_host.py) and against the recordings themselves."""
import numpy as np
import pytest
import torch

import diffsinger_amd
from diffsinger_amd import fs2, hparams
from diffsinger_amd.graphs import GraphedForward
from oracle.fs2_cases import CASES, VOCAB
from tests import fs2_helpers as FH
from tests import regulate_helpers as RH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FREE = ['fs2_lj_free', 'fs2_popcs_free', 'fs2_midi_e2e_free', 'fs2_lj_spkid_energy_free', 'fs2_popcs_ph_free']
FLOAT_KEYS = ('decoder_inp', 'mel_out', 'f0_denorm', 'pitch_pred', 'cwt', 'energy_pred')


def _setup(name):
    case, m, hp, params, inp = FH.case_setup(name)
    m = m.to(DEV)
    tok = inp['txt_tokens'].to(DEV)
    kw = {k: v.to(DEV) for k, v in inp.items() if k != 'txt_tokens'}
    return case, m, tok, kw


@torch.no_grad()
def test_operator_integer_form_equals_the_restatement():
    g = torch.Generator().manual_seed(17)
    n = 0
    for Tt in (1, 2, 63, 64, 65, 300, 4096):
        for alpha in (0.8, 1.0, 1.3):
            for use_pad in (False, True):
                B = int(torch.randint(1, 9, (1,), generator=g))
                dur = torch.randint(1, 41, (B, Tt), generator=g) * (torch.rand(B, Tt, generator=g) > 0.3)
                pad = None
                if use_pad:
                    pad = torch.rand(B, Tt, generator=g) > 0.8
                    pad[B - 1] = True                                               # an all-padded row
                elif B > 1:
                    dur[B - 1] = 0                                                  # a row whose sum is 0
                _, full, want_len = RH.regulate(dur=dur, padding=pad, alpha=alpha)
                longest = max(int(want_len.max()), 1)
                d_dur, d_pad = dur.to(DEV), (pad.to(DEV) if pad is not None else None)
                _, none, len0 = fs2.length_regulate_op(dur=d_dur, dur_padding=d_pad, alpha=alpha)
                assert none is None and len0.dtype == torch.int32 and torch.equal(len0.cpu().long(), want_len)
                for T_out in sorted({longest, longest + 50, longest + 51, max(1, longest // 2), max(1, longest // 2 + 1), 1}):
                    _, want, _ = RH.regulate(dur=dur, padding=pad, alpha=alpha, T_out=T_out)
                    choice, got, got_len = fs2.length_regulate_op(dur=d_dur, dur_padding=d_pad, alpha=alpha, frames=T_out)
                    assert choice is None and got.dtype == torch.int64 and got.shape == (B, T_out)
                    assert torch.equal(got.cpu(), want), (Tt, alpha, use_pad, B, T_out)
                    assert torch.equal(got_len.cpu().long(), want_len), (Tt, alpha, use_pad, B, T_out)          # not clipped to T_out
                    if T_out >= longest and full.shape[1]:
                        assert torch.equal(got.cpu()[:, :full.shape[1]], full) and int(got[:, full.shape[1]:].abs().max() if T_out > full.shape[1] else 0) == 0
                    n += 1
    print(f'{n} (shape, alpha, padding, T_out) cases')
    # the module's own entry: LengthRegulator on device tensors goes through the operator, with and without a budget
    reg = fs2.LengthRegulator()
    dur = torch.randint(0, 9, (3, 40), generator=g)
    pad = torch.rand(3, 40, generator=g) > 0.7
    _, want, _ = RH.regulate(dur=dur, padding=pad, alpha=1.3)
    assert torch.equal(reg(dur.to(DEV), pad.to(DEV), alpha=1.3).cpu(), want)
    assert torch.equal(reg(dur.to(DEV), pad.to(DEV), alpha=1.3, max_frames=want.shape[1] + 9).cpu(), RH.pad_frames(want, want.shape[1] + 9))
    assert reg(torch.zeros(2, 5, dtype=torch.long, device=DEV)).shape == (2, 0)


@pytest.mark.parametrize('name', FREE)
@torch.no_grad()
def test_operator_logdur_form_reproduces_the_recordings(name):
    gold = FH.load_golden(name)
    case = CASES[name]
    from oracle.fs2_cases import make_inputs
    tok = make_inputs(case, False)['txt_tokens']
    logdur = torch.from_numpy(gold['dur'][..., 0]).to(DEV)
    want = torch.from_numpy(gold['mel2ph'])
    T = want.shape[1]
    choice, mel2ph, mel_len = fs2.length_regulate_op(logdur=logdur, offset=1.0, dur_padding=(tok == 0).to(DEV), frames=T)
    want_choice, want_m2p, want_len = RH.regulate(logdur=logdur.cpu(), padding=(tok == 0))
    assert torch.equal(mel2ph.cpu(), want) and torch.equal(choice.cpu(), want_choice) and torch.equal(mel_len.cpu().long(), want_len)
    choice2, none, mel_len2 = fs2.length_regulate_op(logdur=logdur, offset=1.0, dur_padding=(tok == 0).to(DEV))
    assert none is None and torch.equal(choice2, choice) and torch.equal(mel_len2, mel_len)


@torch.no_grad()
def test_operator_out2dur_against_float64_on_two_million_log_durations():
    """Per token, dur_choice equals the float64 out2dur everywhere outside the band where float64 exp(y) - offset lies within 1e-4 of a
    half-integer; inside the band it may differ by 1 at most.  The band is a condition, not a tolerance: it may hold 0.1 % of the tokens at
    most (0.025 % on the CPU for this input; torch's own fp32 exp disagrees with float64 on 3 of the 2e6, all inside the band)."""
    g = torch.Generator().manual_seed(23)
    B, Tt = 500, 4000
    y = torch.rand(B, Tt, generator=g) * 4.5 - 1.0
    want = RH.out2dur64(y)
    band = RH.half_distance64(y) < 1e-4
    share = float(band.double().mean())
    choice, _, mel_len = fs2.length_regulate_op(logdur=y.to(DEV), offset=1.0)
    got = choice.cpu()
    diff = (got - want).abs()
    outside, inside = int(diff[~band].max()), int(diff[band].max() if band.any() else 0)
    print(f'band share {share:.5%}; mismatches outside the band {int((diff[~band] != 0).sum())}, inside {int((diff[band] != 0).sum())} of {int(band.sum())}')
    assert share <= 1e-3
    assert outside == 0 and inside <= 1
    assert torch.equal(mel_len.cpu().long(), got.sum(-1))
    torch_dev = torch.clamp(torch.round(y.to(DEV).exp() - 1.0), min=0).long().cpu()                   # the reference path on this device
    print(f'operator vs torch device ops: {int((torch_dev != got).sum())} of {got.numel()} tokens differ')


@torch.no_grad()
def test_operator_non_finite_log_durations_follow_the_header():
    y = torch.tensor([[float('nan'), 0.0, float('inf'), 1.0, float('-inf'), 100.0, 2.0, -5.0]])
    choice, mel2ph, mel_len = fs2.length_regulate_op(logdur=y.to(DEV), offset=1.0, frames=64)
    cap = 1 << 20
    assert choice.cpu().tolist() == [[0, 0, cap, 2, 0, cap, 6, 0]]                                   # NaN counts as 0; a token saturates at 1 << 20
    assert int(mel_len[0]) == 2 * cap + 8
    assert mel2ph.cpu()[0].tolist() == [3] * 64                                                      # NaN and the zero tokens own no frame
    dur = torch.tensor([[-3, 2, 1 << 40, 1]])
    _, mel2ph, mel_len = fs2.length_regulate_op(dur=dur.to(DEV), frames=5)
    assert mel2ph.cpu()[0].tolist() == [2, 2, 3, 3, 3] and int(mel_len[0]) == 2 + cap + 1            # negative -> 0, saturation
    big = torch.full((1, 4096), 1 << 30)
    _, _, mel_len = fs2.length_regulate_op(dur=big.to(DEV), alpha=1.3)
    assert int(mel_len[0]) == 2 ** 31 - 1                                                            # the row sum saturates, it does not wrap
    torch.cuda.synchronize()


def _pair(name):
    """(budgeted free-running forward, teacher-forced forward on the padded recording, recording, N)."""
    case, m, tok, kw = _setup(name)
    gold = FH.load_golden(name)
    g_m2p = torch.from_numpy(gold['mel2ph'])
    N = g_m2p.shape[1] + 37
    padded = RH.pad_frames(g_m2p, N).to(DEV)
    free = m(tok, infer=True, max_frames=N, **kw)
    teacher = m(tok, mel2ph=padded, infer=True, **kw)
    torch.cuda.synchronize()
    return free, teacher, gold, padded, N


@pytest.mark.parametrize('name', FREE)
@torch.no_grad()
def test_budgeted_free_running_forward_equals_the_teacher_forced_forward_bitwise(name):
    """Past add_dur both calls run the same operators on the same shapes and the same integers: every output carries the same bits."""
    free, teacher, gold, padded, N = _pair(name)
    assert free['mel2ph'].dtype == torch.int64 and torch.equal(free['mel2ph'], padded)
    assert free['mel_len'].dtype == torch.int32 and torch.equal(free['mel_len'].cpu().long(), torch.from_numpy((gold['mel2ph'] > 0).sum(-1)))
    assert free['dur_choice'].dtype == torch.int64
    assert free['dur'].shape == teacher['dur'].shape + (1,) and torch.equal(free['dur'][..., 0], teacher['dur'])
    checked = []
    for k in FLOAT_KEYS:
        if k in teacher or k in free:
            assert torch.equal(free[k], teacher[k]), (name, k, float((free[k] - teacher[k]).abs().max()))
            checked.append(k)
    assert 'decoder_inp' in checked and 'mel_out' in checked
    assert free['mel_out'].shape[:2] == (padded.shape[0], N)
    pad = padded == 0
    assert float(free['decoder_inp'][pad].abs().max()) == 0 and float(free['mel_out'][pad].abs().max()) == 0


@pytest.mark.parametrize('name', FREE)
@torch.no_grad()
def test_budgeted_free_running_forward_against_the_recordings(name):
    """The first T_golden frames against the reference's recording at the suite's bound for the whole model (tests/test_gpu_fs2.py: 1e-4
    max-abs), frames past a row's length exactly 0.  This holds because the columns behind the longest row count as the end of the tensor
    (fs2.frame_keep): in the reference's arithmetic a padding frame enters the k > 1 convolution behind a LayerNorm as the LayerNorm's bias,
    so without that mask the 37 spare columns move mel_out by 3e-2 (measured on one MI355X before the mask was built)."""
    free, teacher, gold, padded, N = _pair(name)
    T = gold['mel2ph'].shape[1]
    np.testing.assert_array_equal(free['mel2ph'].cpu().numpy()[:, :T], gold['mel2ph'])
    pad = padded == 0
    assert float(free['decoder_inp'][pad].abs().max()) == 0 and float(free['mel_out'][pad].abs().max()) == 0
    errs = {}
    for k in ('dur', 'decoder_inp', 'mel_out', 'pitch_pred', 'cwt', 'energy_pred', 'f0_denorm'):
        if k not in gold:
            continue
        got = free[k].cpu().numpy()
        got = got if k == 'dur' else got[:, :T]
        scale = np.maximum(np.abs(gold[k]), 1.0) if k == 'f0_denorm' else 1.0          # Hz: relative, as tests/test_gpu_fs2.py measures it
        errs[k] = float((np.abs(got - gold[k]) / scale).max())
        print(f'{name}:{k}: max-abs err vs the recording on the first {T} of {N} frames {errs[k]:.3e} (max|ref| {float(np.abs(gold[k]).max()):.2f})')
    assert all(e <= 1e-4 for e in errs.values()), (name, errs)


@pytest.mark.parametrize('name', FREE)
@torch.no_grad()
def test_without_a_budget_nothing_changes(name):
    """max_frames=None: the operator path (one launch for the lengths, the host read, one launch for mel2ph), the operator on torch's
    out2dur and the torch sequence it replaces give the same integers and the same bits everywhere."""
    case, m, tok, kw = _setup(name)
    gold = FH.load_golden(name)
    outs = {}
    try:
        for label, sw in (('native', dict(regulate=True, exp=True)), ('torch_exp', dict(regulate=True, exp=False)), ('torch', dict(regulate=False))):
            fs2.set_regulate_native(**sw)
            outs[label] = m(tok, infer=True, **kw)
            torch.cuda.synchronize()
    finally:
        fs2.set_regulate_native(True, True)
    base = outs['torch']
    np.testing.assert_array_equal(base['mel2ph'].cpu().numpy(), gold['mel2ph'])
    for label in ('native', 'torch_exp'):
        o = outs[label]
        assert set(o) == set(base)
        for k in sorted(base):
            if torch.is_tensor(base[k]):
                assert o[k].dtype == base[k].dtype and o[k].shape == base[k].shape and torch.equal(o[k], base[k]), (label, k)
    assert base['mel_len'].dtype == torch.int32 and torch.equal(base['mel_len'].cpu().long(), torch.from_numpy((gold['mel2ph'] > 0).sum(-1)))


@pytest.mark.parametrize('name', ['fs2_popcs_free', 'fs2_midi_e2e_free'])
@torch.no_grad()
def test_budgeted_forward_is_captured_once_and_follows_new_tokens(name):
    """No host read, shown by capture: one graph, replayed on OTHER tokens of the same shape (other durations, other lengths), carries the bits
    of the eager call on those tokens."""
    case, m, tok, kw = _setup(name)
    gold = FH.load_golden(name)
    N = gold['mel2ph'].shape[1] + 37
    keys = sorted(kw)
    gm = GraphedForward(lambda t, *vals: m(t, infer=True, max_frames=N, **dict(zip(keys, vals))))
    g = torch.Generator().manual_seed(99)
    tok_b = torch.where(tok > 0, torch.randint(1, VOCAB, tok.shape, generator=g).to(DEV), tok)
    seen = []
    for t in (tok, tok_b, tok):
        want = {k: v.clone() for k, v in m(t, infer=True, max_frames=N, **kw).items() if torch.is_tensor(v)}
        got = gm(t, *[kw[k] for k in keys])
        for k, v in want.items():
            assert torch.equal(got[k], v), (name, k)
        seen.append(want)
    assert gm.captures == 1
    assert not torch.equal(seen[0]['mel2ph'], seen[1]['mel2ph']) and not torch.equal(seen[0]['mel_len'], seen[1]['mel_len'])


@torch.no_grad()
def test_diffusion_forward_on_a_budget():
    name = 'fs2_popcs_free'
    case, m, tok, kw = _setup(name)
    gold = FH.load_golden(name)
    from diffsinger_amd.synth import presets
    pre = presets()[case['preset']]
    net = diffsinger_amd.DIFF_DECODERS['wavenet'](hparams)
    torch.manual_seed(3)
    torch.nn.init.normal_(net.output_projection.weight, std=0.02)
    gd = diffsinger_amd.GaussianDiffusion(None, 80, net, timesteps=pre['timesteps'], K_step=4, loss_type='l1', spec_min=pre['spec_min'],
                                          spec_max=pre['spec_max'], fs2=m).to(DEV).eval()
    g_m2p = torch.from_numpy(gold['mel2ph'])
    T = g_m2p.shape[1]
    N = T + 37
    padded = RH.pad_frames(g_m2p, N).to(DEV)
    torch.manual_seed(11)
    free = gd(tok, infer=True, max_frames=N, **kw)
    torch.manual_seed(11)
    teacher = gd(tok, mel2ph=padded, infer=True, **kw)
    assert free['mel_out'].shape == (tok.shape[0], N, 80)
    assert torch.equal(free['mel_out'], teacher['mel_out']) and torch.equal(free['fs2_mel'], teacher['fs2_mel'])
    assert bool(torch.isfinite(free['mel_out']).all()) and float(free['mel_out'][padded > 0].abs().max()) > 0
    assert float(free['mel_out'][padded == 0].abs().max()) == 0
    assert torch.equal(free['mel_len'].cpu().long(), (g_m2p > 0).sum(-1))
    with pytest.raises(RuntimeError, match=str(T)):
        gd(tok, infer=True, max_frames=T - 5, **kw)
    with pytest.raises(ValueError):
        gd(tok, infer=True, max_frames=0, **kw)


@torch.no_grad()
def test_two_eager_calls_are_bitwise_equal():
    case, m, tok, kw = _setup('fs2_lj_free')
    N = FH.load_golden('fs2_lj_free')['mel2ph'].shape[1] + 37
    a = {k: v.clone() for k, v in m(tok, infer=True, max_frames=N, **kw).items() if torch.is_tensor(v)}
    b = m(tok, infer=True, max_frames=N, **kw)
    for k, v in a.items():
        assert torch.equal(b[k], v), k
    g = torch.Generator().manual_seed(1)
    y = (torch.rand(8, 4096, generator=g) * 4.5 - 1.0).to(DEV)
    r1 = fs2.length_regulate_op(logdur=y, frames=200001)
    r2 = fs2.length_regulate_op(logdur=y, frames=200001)
    assert all(torch.equal(p, q) for p, q in zip(r1, r2))
