"""GPU: the FastSpeech2 training objective on HIP (diffsinger_amd/losses.py, csrc/fs2_loss.hpp) - the fused mel L1 + SSIM and the duration terms
against the restated reference (tests/fs2_loss_helpers.py) in fp32 and float64, the whole objective with the decoder trained (skip_decoder=False)
against oracle/fs2_oracle.py under autograd, determinism, graph capture and the refusals."""
import pytest
import torch

from diffsinger_amd import _lib, losses
from tests import fs2_loss_helpers as LH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max() / max(float(b.detach().abs().max()), 1e-30))


def test_new_abi_symbols_exist():
    lib = _lib.load()
    for name in ('dsf_mel_loss', 'dsf_mel_loss_bwd', 'dsf_dur_loss', 'dsf_dur_loss_bwd', 'dsf_fs2_loss_workspace_floats'):
        assert hasattr(lib, name), name
    assert lib.dsf_fs2_loss_workspace_floats(2, 37, 0) == 2 * 3 * 4


@pytest.mark.parametrize('B,T,M,bias', [(1, 5, 80, 6.0), (2, 37, 80, 6.0), (3, 300, 80, 6.0), (8, 1024, 80, 6.0), (1, 8000, 80, 6.0), (2, 200, 10, 20.0)])
def test_mel_l1_ssim_values_and_gradient(B, T, M, bias):
    x, y = LH.mel_case(B, T, M, seed=B * 1000 + T + M, bias_scale=1.0 if M == 80 else 0.5)
    # reference fp32 and float64 (CPU autograd)
    ref = {}
    for dt in (torch.float32, torch.float64):
        xr = x.detach().to(dt).clone().requires_grad_(True)
        l1, ss = LH.l1_loss(xr, y.to(dt)), LH.ssim_loss(xr, y.to(dt), bias)
        (0.5 * l1 + 0.5 * ss).backward()
        ref[dt] = (float(l1), float(ss), xr.grad)
    xd = x.to(DEV).requires_grad_(True)
    out = losses.mel_loss_terms(xd, y.to(DEV), bias=bias, lam_l1=0.5, lam_ssim=0.5)
    (out[0] + out[1]).backward()
    l1_32, ss_32, g32 = ref[torch.float32]
    l1_64, ss_64, g64 = ref[torch.float64]
    e_l1 = abs(float(out[0]) / 0.5 - l1_32) / abs(l1_32)
    e_ss = abs(float(out[1]) / 0.5 - ss_32) / abs(ss_32)
    e_g, e_g32 = _rel(xd.grad, g64), _rel(g32, g64)
    print(f'mel loss B={B} T={T} M={M}: l1 rel {e_l1:.1e}, ssim rel {e_ss:.1e} (vs fp64: {abs(float(out[1]) / 0.5 - ss_64) / abs(ss_64):.1e}), '
          f'grad vs fp64 {e_g:.1e} (reference fp32: {e_g32:.1e})')
    assert e_l1 <= 1e-5 and e_g <= max(2 * e_g32, 2e-7)
    if M == 80:
        assert e_ss <= 1e-5 and e_g <= 1e-5
    else:
        # bias 20 on cwt-like values: E11 ~ 400 beside variances ~ 0.1, so fp32 itself is ~1e-4 from float64 (the reference's fp32 included);
        # the bar is then the reference fp32's own distance from float64
        e64, e32_64 = abs(float(out[1]) / 0.5 - ss_64) / abs(ss_64), abs(ss_32 - ss_64) / abs(ss_64)
        assert e64 <= max(2 * e32_64, 1e-5) and e_g <= 2 * e_g32


def test_ssim_dropin_map_mean_and_gradient():
    x, y = LH.mel_case(2, 120, 80, seed=5)
    a, b = x[:, None] + 6.0, y[:, None] + 6.0
    want = LH.ssim_map(a.double(), b.double())
    m = losses.ssim(a.to(DEV), b.to(DEV), size_average=False)
    assert m.shape == (2, 120, 80)
    assert _rel(m, want.mean(1)) <= 1e-5
    ad = a.to(DEV).requires_grad_(True)
    s = losses.ssim(ad, b.to(DEV))
    ar = a.double().requires_grad_(True)
    sr = LH.ssim_map(ar, b.double()).mean()
    sr.backward()
    s.backward()
    assert abs(float(s) - float(sr)) <= 1e-5 * abs(float(sr))
    m32 = a.clone().requires_grad_(True)
    LH.ssim_map(m32, b).mean().backward()
    e, e32 = _rel(ad.grad, ar.grad), _rel(m32.grad, ar.grad)
    print(f'ssim mean gradient vs fp64 {e:.1e} (reference fp32: {e32:.1e})')
    assert e <= max(2 * e32, 1e-5)
    # the map's own gradient path: sum(map * R)
    R = torch.randn(2, 120, 80, generator=torch.Generator().manual_seed(3))
    ad.grad = None
    (losses.ssim(ad, b.to(DEV), size_average=False) * R.to(DEV)).sum().backward()
    ar.grad = None
    (LH.ssim_map(ar, b.double()).mean(1) * R.double()).sum().backward()
    a32 = a.clone().requires_grad_(True)
    (LH.ssim_map(a32, b).mean(1) * R).sum().backward()
    e, e32 = _rel(ad.grad, ar.grad), _rel(a32.grad, ar.grad)
    print(f'ssim map gradient vs fp64 {e:.1e} (reference fp32: {e32:.1e})')
    assert e <= max(2 * e32, 1e-5)


def _dur_case(seed):
    """3 utterances, 12 phones: a phone with zero frames, padded phones, a row without silence phones (sil ids 1, 2, 7)."""
    g = torch.Generator().manual_seed(seed)
    B, Tt = 3, 12
    tok = torch.randint(8, 40, (B, Tt), generator=g)
    tok[0, [0, 4, 9]] = torch.tensor([1, 7, 2])                       # silences in row 0
    tok[1, 3] = 7
    tok[1, 9:] = 0                                                    # padding
    tok[2, 10:] = 0                                                   # row 2: no silence phone
    dur = torch.randint(1, 6, (B, Tt), generator=g) * (tok > 0)
    dur[0, 6] = 0                                                     # a phone with no frame
    dur[2, 2] = 0
    T = int(dur.sum(-1).max()) + 3                                    # padding frames at the end of every row
    mel2ph = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        t = 0
        for i in range(Tt):
            mel2ph[b, t:t + int(dur[b, i])] = i + 1
            t += int(dur[b, i])
    dur_pred = torch.randn(B, Tt, generator=g) * 0.6 + 1.0
    wdb = (torch.rand(B, Tt, generator=g) < 0.4).long() * (tok > 0)
    wdb[:, -1] = 0
    return dur_pred, mel2ph, tok, dur, wdb


@pytest.mark.parametrize('seg', ['sil', 'word_boundary'])
def test_duration_terms_values_and_gradient(seg):
    dur_pred, mel2ph, tok, dur, wdb = _dur_case(11)
    sil = [1, 2, 7]
    kw = dict(sil_ids=sil) if seg == 'sil' else dict(wdb=wdb)
    lam = dict(lam_ph=0.7 if seg == 'sil' else 1.0, lam_word=1.3, lam_sent=0.9)
    dr = dur_pred.double().requires_grad_(True)
    want = LH.dur_loss(dr, mel2ph, tok, **kw, **lam)
    sum(want.values()).backward()
    # durations are integers, bit-exact
    assert torch.equal(LH.mel2ph_to_dur(mel2ph, tok.shape[1]) * (tok > 0), dur * (tok > 0))
    dd = dur_pred.to(DEV).requires_grad_(True)
    kd = dict(sil_ids=torch.tensor(sil, device=DEV)) if seg == 'sil' else dict(word_boundary=wdb.to(DEV))
    out = losses.dur_loss_terms(dd, mel2ph.to(DEV), tok.to(DEV), **kd, **lam)
    out.sum().backward()
    got = dict(zip(('pdur', 'wdur', 'sdur'), out.detach().cpu().tolist()))
    print(f'dur terms ({seg}): {got} vs {({k: float(v) for k, v in want.items()})}, grad rel {_rel(dd.grad, dr.grad):.1e}')
    for k, v in want.items():
        assert abs(got[k] - float(v)) <= 1e-6 * max(abs(float(v)), 1e-3), k
    assert _rel(dd.grad, dr.grad) <= 1e-6


def test_mel2ph_out_of_range_gives_nan_and_bad_input_raises():
    dur_pred, mel2ph, tok, dur, wdb = _dur_case(12)
    bad = mel2ph.clone()
    bad[1, 2] = tok.shape[1] + 1
    out = losses.dur_loss_terms(dur_pred.to(DEV), bad.to(DEV), tok.to(DEV), word_boundary=wdb.to(DEV))
    assert torch.isnan(out).all()
    with pytest.raises(ValueError):
        losses.dur_loss_terms(dur_pred, mel2ph, tok, word_boundary=wdb)                 # CPU tensors
    with pytest.raises(ValueError):
        losses.mel_loss_terms(torch.zeros(1, 5, 80), torch.zeros(1, 5, 80))              # CPU tensors
    with pytest.raises(ValueError):
        losses.mel_loss_terms(torch.zeros(1, 5, 129, device=DEV), torch.zeros(1, 5, 129, device=DEV))
    with pytest.raises(ValueError):
        losses.ssim(torch.zeros(1, 2, 5, 80, device=DEV), torch.zeros(1, 2, 5, 80, device=DEV))
    with pytest.raises(ValueError):
        losses.ssim(torch.zeros(1, 1, 5, 80, device=DEV), torch.zeros(1, 1, 5, 80, device=DEV), window_size=7)


def _objective_step(x, y, dur_pred, mel2ph, tok, wdb):
    out = losses.mel_loss_terms(x, y, lam_l1=0.5, lam_ssim=0.5)
    d = losses.dur_loss_terms(dur_pred, mel2ph, tok, word_boundary=wdb)
    loss = out[0] + out[1] + d.sum()
    loss.backward()
    return loss


def test_determinism_and_graph_capture():
    x, y = LH.mel_case(4, 333, 80, seed=77)
    dur_pred, mel2ph, tok, dur, wdb = _dur_case(13)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    dd = dur_pred.to(DEV).requires_grad_(True)
    args = (xd, yd, dd, mel2ph.to(DEV), tok.to(DEV), wdb.to(DEV))
    l_a = _objective_step(*args).detach().clone()
    gx_a, gd_a = xd.grad.clone(), dd.grad.clone()
    xd.grad, dd.grad = None, None
    l_b = _objective_step(*args).detach().clone()
    assert torch.equal(l_a, l_b) and torch.equal(gx_a, xd.grad) and torch.equal(gd_a, dd.grad)
    # captured: no host synchronisation anywhere in forward + backward
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xd.grad, dd.grad = None, None
            _objective_step(*args)
    torch.cuda.current_stream().wait_stream(s)
    xd.grad, dd.grad = None, None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        l_c = _objective_step(*args)
    xd.grad.zero_()
    dd.grad.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(l_c.detach(), l_a) and torch.equal(xd.grad, gx_a) and torch.equal(dd.grad, gd_a)


# ---- the whole objective with the decoder trained ----------------------------------------------------------------------------------------
LOSS_HP = {'dur_loss': 'mse', 'pitch_loss': 'l1', 'lambda_ph_dur': 1.0, 'lambda_word_dur': 1.0, 'lambda_sent_dur': 1.0, 'lambda_f0': 1.0,
           'lambda_uv': 1.0, 'lambda_energy': 0.1, 'cwt_loss': 'l1', 'cwt_add_f0_loss': False}
OBJ_CASES = {'fs2_lj_teacher': ('fs2', 'l1'), 'fs2_popcs_teacher': ('fs2', 'ssim:0.5|l1:0.5'), 'fs2_popcs_ph_teacher': ('fs2', 'ssim:0.5|l1:0.5'),
             'fs2_popcs_spk_energy_teacher': ('fs2', 'ssim:0.5|l1:0.5'), 'fs2_midi_cascade_teacher': ('midi', 'ssim:0.5|l1:0.5')}
SIL = [1, 2, 5, 9]


def _sample(case, inp):
    g = torch.Generator().manual_seed(case['seed'] + 500)
    mel2ph, tok = inp['mel2ph'], inp['txt_tokens']
    B, T = mel2ph.shape
    s = {'txt_tokens': tok, 'mel2ph': mel2ph, 'mels': (torch.randn(B, T, 80, generator=g) * 1.2 - 4.0) * (mel2ph > 0)[:, :, None]}
    for k in ('f0', 'uv', 'energy'):
        if k in inp:
            s[k] = inp[k]
    s['cwt_spec'] = torch.randn(B, T, 10, generator=g)
    s['f0_mean'] = torch.rand(B, generator=g) * 2 + 6.5
    s['f0_std'] = torch.rand(B, generator=g) * 0.5 + 0.2
    wdb = (torch.rand(tok.shape, generator=g) < 0.5).long() * (tok > 0)
    s['word_boundary'] = wdb
    return s


def _objective_reference(o, s, hp, variant):
    """FastSpeech2Task / AuxDecoderMIDITask.run_model's losses (tasks/tts/fs2.py:111-283, usr/diffsinger_task.py:404-473) restated on torch."""
    import torch.nn.functional as F
    L = {}
    for k, lbd in losses.parse_mel_loss(hp['mel_loss']).items():
        L[k] = (LH.l1_loss(o['mel_out'], s['mels']) if k == 'l1' else LH.ssim_loss(o['mel_out'], s['mels'])) * lbd
    kw = dict(sil_ids=SIL, lam_ph=hp['lambda_ph_dur']) if variant == 'fs2' else dict(wdb=s['word_boundary'], lam_ph=1.0)
    L.update(LH.dur_loss(o['dur'], s['mel2ph'], s['txt_tokens'], lam_word=hp['lambda_word_dur'], lam_sent=hp['lambda_sent_dur'], **kw))

    def mm(v, m):
        return (v * m).sum() / m.sum()
    if hp.get('use_pitch_embed'):
        if hp['pitch_type'] == 'ph':
            L['f0'] = mm(F.l1_loss(o['pitch_pred'][:, :, 0], s['f0'], reduction='none'), (s['txt_tokens'] != 0).float()) * hp['lambda_f0']
        else:
            npd = (s['mel2ph'] != 0).float()
            if hp['pitch_type'] == 'cwt':
                L['C'] = F.l1_loss(o['cwt'][:, :, :10], s['cwt_spec']) * hp['lambda_f0']
                L['uv'] = mm(F.binary_cross_entropy_with_logits(o['cwt'][:, :, -1], s['uv'], reduction='none'), npd) * hp['lambda_uv']
                L['f0_mean'] = F.l1_loss(o['f0_mean'], s['f0_mean']) * hp['lambda_f0']
                L['f0_std'] = F.l1_loss(o['f0_std'], s['f0_std']) * hp['lambda_f0']
            else:
                L['uv'] = mm(F.binary_cross_entropy_with_logits(o['pitch_pred'][:, :, 1], s['uv'], reduction='none'), npd) * hp['lambda_uv']
                npd = npd * (s['uv'] == 0).float()
                L['f0'] = mm(F.l1_loss(o['pitch_pred'][:, :, 0], s['f0'], reduction='none'), npd) * hp['lambda_f0']
    if hp.get('use_energy_embed'):
        L['e'] = mm(F.mse_loss(o['energy_pred'], s['energy'], reduction='none'), (s['energy'] != 0).float()) * hp['lambda_energy']
    return L


@pytest.mark.parametrize('name', list(OBJ_CASES))
def test_whole_objective_with_the_decoder_trained(name):
    from oracle import fs2_oracle as FO
    from tests import fs2_helpers as FH
    variant, mel_loss = OBJ_CASES[name]
    case, m, hp, params, inp = FH.case_setup(name)
    hp = dict(hp, **LOSS_HP, mel_loss=mel_loss)
    s = _sample(case, inp)
    p = FH.oracle_params(params)
    kw = {k: v.clone() for k, v in inp.items() if k != 'txt_tokens'}
    o = FO.fs2_forward(p, hp, inp['txt_tokens'], skip_decoder=False, **kw)
    want = _objective_reference(o, s, hp, variant)
    sum(want.values()).backward()
    m = m.to(DEV).eval()
    kw = {k: v.clone().to(DEV) for k, v in inp.items() if k != 'txt_tokens'}
    r = m(inp['txt_tokens'].to(DEV), skip_decoder=False, infer=False, **kw)
    sd = {k: v.to(DEV) for k, v in s.items()}
    got = losses.fs2_losses(r, sd, hp, variant=variant, sil_ph_ids=torch.tensor(SIL, device=DEV))
    assert list(got) == list(want), (list(got), list(want))
    sum(got.values()).backward()
    e_val = {k: abs(float(got[k]) - float(want[k])) / max(abs(float(want[k])), 1e-3) for k in want}
    alias = {'encoder.embed_tokens.weight', 'encoder_embed_tokens.weight'}
    worst, n, dec = ('', 0.0), 0, 0
    for k, prm in m.named_parameters():
        parts = [p[a].grad for a in (alias if k in alias else {k}) if a in p and p[a].grad is not None]
        if not parts:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, f'{k}: gradient where the oracle has none'
            continue
        assert prm.grad is not None, f'{k}: no gradient'
        e = _rel(prm.grad, sum(parts))
        n += 1
        dec += k.startswith(('decoder.', 'mel_out.'))
        if e > worst[1]:
            worst = (k, e)
    print(f'{name}: {({k: round(float(v), 6) for k, v in got.items()})}, worst value err {max(e_val.values()):.1e}, {n} gradients ({dec} decoder / '
          f'mel_out), worst rel err {worst[1]:.2e} at {worst[0]}')
    assert all(v <= 1e-5 for v in e_val.values()), e_val
    assert dec >= 10 and worst[1] <= 5e-6, worst
