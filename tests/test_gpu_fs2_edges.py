"""The FFT-block operators of include/dsf.h (attention core, LayerNorm, convolution, layout changes) on the MI355X at the lengths and score
ranges the mel-rate decoder runs at, against float64 restatements with element-wise conditions (tests/fs2_ops_helpers.py; the conditions
themselves are judged on the CPU by tests/test_fs2_ops_host.py).

Attention forward: every score profile of fs2_ops_helpers.KINDS at every length of fs2_ops_helpers.SHAPES - up to nine key tiles per wave,
raises of the lazy reference maximum after a wave's first tile, P > 1 against an un-raised maximum, waves that start on dead tiles, padded keys
inside live tiles, a dead stretch in the middle - |device - O64| <= bound element-wise, zero tail; 1 and 3 heads, no key mask, bitwise
repeatability and batch independence; an utterance whose keys are ALL padded gives exactly 0 (torch gives NaN) and leaves the others' bits alone.
Attention backward: T = 257, 300, 520 (the second pass of the row kernels' 256-wide loops) against float64 autograd by the yardstick.
LayerNorm: both kernels (C = 256; 248, 80, 8), T around the 32-frame tile, large mean with small spread, an outlier channel, tiny inputs.
Convolution: both kernels at the full halo, fewer frames than the reach, short second channel slabs, mish, gelu with a scale; refusals.
One whole FastSpeech2 forward at about 1050 frames against the CPU oracle.

MEASURED on the MI355X, 2026-10-19 (every case passes; no kernel was changed).  "share" = largest |device - float64| / bound over the elements of
every case; "ratio" = the device's largest error / the float32 CPU evaluation's (information only).
  attention forward, share of the bound (ratio) per kind over all 11 shapes:
      flat 0.041 (1.35)   ramp_up_fast 0.176 (1.35)   ramp_up_slow 0.112 (1.22)   ramp_down 0.157 (1.23)   spike 0.044 (8.06)   offset 0.133 (1.16)
      (spike: the fp32 CPU softmax is nearly exact where one key takes all the weight; the device's error there is 1e-6 absolute)
      heads = 1: 0.081 (1.07), heads = 3: 0.112 (0.89); no key mask: T = 45 0.036 (0.94), T = 257 0.072 (1.04)
  attention backward, largest rel_err over T = 257, 300, 520 (ratio); allowed max(4 x fp32 CPU, 1e-5) = 1e-5 ... 3.2e-5:
      flat o 1.0e-6 (1.24) dqkv 9.6e-7 (1.50)   ramp_up_fast o 7.0e-6 (1.02) dqkv 4.5e-6 (1.23)   spike o 7.2e-7 (1.34) dqkv 7.0e-7 (2.01)
  LayerNorm, share of the allowed error max(4 x fp32 CPU, 2e-6) (ratio), per kind as C = 256 / 248 / 80 / 8:
      plain 0.095 / 0.105 / 0.085 / 0.099 (<= 1.86)   offset 0.406 / 0.912 / 0.358 / 0.326 (<= 3.65; rel_err up to 6e-5 on either side: the mean of
      values near 100 is rounded to 8e-6)   outlier 0.241 / 0.199 / 0.123 / 0.098 (<= 3.16)   small 0.130 / 0.123 / 0.096 / 0.106 (<= 2.30)
  convolution, share of the bound, k_fs_conv / k_fs_conv_ks: 0.060 ... 0.239 / 0.060 ... 0.084 (ratio 0.74 ... 5.92 / 0.32 ... 2.19: the 256-row kernel
      is one sequential chain per output, aten's blocked sum is more accurate than either); mish 0.239 / 0.077, gelu with scale 1/3 0.196 / 0.074
  whole FastSpeech2 at 1084 frames (2 x 300 phones), max-abs error against the CPU oracle, tolerance 1e-4:
      dur 2.4e-6   cwt 3.8e-6   decoder_inp 1.7e-6   mel_out 2.4e-6   mel2ph exact
"""
import pytest
import torch
import torch.nn.functional as F

from tests import fs2_helpers as FH
from tests import fs2_ops_helpers as OH

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def _u8(pad):
    return None if pad is None else pad.to(torch.uint8).to(DEV).contiguous()


def _attention_cm(qkv, pad, heads):
    """the device's channel-major output [B][C][TS] for [B, T, 3C] inputs on the CPU"""
    from diffsinger_amd import fs2
    with torch.no_grad():
        return fs2.attention_cm(fs2.to_cm(qkv.to(DEV)), qkv.shape[1], _u8(pad), heads)


def _attention(qkv, pad, heads):
    """([B, T, C] on the CPU, largest |value| of the tail [T, TS))"""
    from diffsinger_amd import fs2
    T = qkv.shape[1]
    out = _attention_cm(qkv, pad, heads)
    assert out.shape == (qkv.shape[0], OH.HD * heads, fs2.padded_frames(T))
    tail = float(out[:, :, T:].abs().max()) if out.shape[2] > T else 0.0
    return fs2.from_cm(out, T).cpu(), tail


def _judge_attention(tag, qkv, pad, heads):
    o64, bnd = OH.attention64(qkv, pad, heads)
    o32 = OH.attention_ref(qkv, pad, heads, torch.float32)[0]
    got, tail = _attention(qkv, pad, heads)
    share = OH.used(got, o64, bnd)
    e_dev, e_cpu = float((got.double() - o64).abs().max()), float((o32.double() - o64).abs().max())
    print(f'EDGE attention {tag}: uses {share:.3f} of the bound; max err {e_dev:.2e} (bound there <= {float(bnd.max()):.2e}), '
          f'device / fp32-CPU error {e_dev / max(e_cpu, 1e-300):.2f}')
    assert bool(torch.isfinite(got).all())
    assert share <= 1.0
    assert tail == 0.0


# ---- attention forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', OH.SHAPES)
@pytest.mark.parametrize('kind', OH.KINDS)
def test_attention_forward(kind, B, T):
    qkv, pad = OH.attention_inputs(kind, B, T, OH.seed_of(T))
    _judge_attention(f'kind={kind} B={B} T={T}', qkv, pad, 2)


@pytest.mark.parametrize('heads', [1, 3])
def test_attention_forward_heads(heads):
    qkv, pad = OH.attention_inputs('ramp_up_fast', 2, 160, OH.seed_of(160), heads=heads)
    _judge_attention(f'heads={heads} kind=ramp_up_fast B=2 T=160', qkv, pad, heads)


@pytest.mark.parametrize('B,T', [(2, 45), (2, 257)])
def test_attention_forward_without_a_key_mask(B, T):
    qkv, _ = OH.attention_inputs('ramp_up_slow', B, T, OH.seed_of(T))
    _judge_attention(f'key_pad=None kind=ramp_up_slow B={B} T={T}', qkv, None, 2)


def test_attention_is_repeatable_and_independent_of_the_batch():
    """Two calls carry the same bits; a workgroup is one (query tile, head, utterance), so utterance 0 alone carries the bits of its row."""
    qkv, pad = OH.attention_inputs('ramp_up_fast', 3, 257, OH.seed_of(257))
    a, b = _attention_cm(qkv, pad, 2), _attention_cm(qkv, pad, 2)
    assert torch.equal(a, b)
    alone = _attention_cm(qkv[:1], pad[:1], 2)
    assert torch.equal(alone[0], a[0])


def test_attention_of_an_utterance_whose_keys_are_all_padded():
    """Pinned as it is: such an utterance's output is exactly 0 (the torch expression gives NaN there), and the other utterances carry the bits
    they carry without it."""
    B, T = 3, 70
    qkv, pad = OH.attention_inputs('flat', B, T, OH.seed_of(T))
    pad[1, :] = True
    assert bool(torch.isnan(OH.attention_ref(qkv, pad, 2, torch.float32)[0][1]).all())
    out = _attention_cm(qkv, pad, 2)
    assert float(out[1].abs().max()) == 0.0
    assert float(out[:, :, T:].abs().max()) == 0.0
    others = _attention_cm(qkv[[0, 2]], pad[[0, 2]], 2)
    assert torch.equal(out[[0, 2]], others)
    from diffsinger_amd import fs2
    o64, bnd = OH.attention64(qkv[[0, 2]], pad[[0, 2]], 2)
    assert OH.used(fs2.from_cm(others, T).cpu(), o64, bnd) <= 1.0


# ---- attention backward ------------------------------------------------------------------------------------------------------------------------
def _attention_autograd(qkv, pad, do, heads, dtype):
    r = qkv.detach().to(dtype).clone().requires_grad_(True)
    B, T, _ = qkv.shape
    q, k, v = [t.reshape(B, T, heads, OH.HD).transpose(1, 2) for t in r.chunk(3, -1)]
    s = (q * torch.tensor(OH.scale64(), dtype=dtype)) @ k.transpose(-1, -2)
    s = s.masked_fill(pad[:, None, None, :], float('-inf'))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, OH.HD * heads)
    o.backward(do.to(dtype))
    return o.detach(), r.grad


@pytest.mark.parametrize('B,T', [(2, 257), (2, 300), (1, 520)])
@pytest.mark.parametrize('kind', ['flat', 'ramp_up_fast', 'spike'])
def test_attention_backward(kind, B, T):
    from diffsinger_amd import fs2
    qkv, pad = OH.attention_inputs(kind, B, T, OH.seed_of(T))
    do = torch.randn(B, T, 2 * OH.HD, generator=torch.Generator().manual_seed(T + 5))
    o64, d64 = _attention_autograd(qkv, pad, do, 2, torch.float64)
    o32, d32 = _attention_autograd(qkv, pad, do, 2, torch.float32)
    qc = fs2.to_cm(qkv.to(DEV)).requires_grad_(True)
    out = fs2.attention_cm(qc, T, _u8(pad), 2)
    out.backward(fs2.to_cm(do.to(DEV)))
    got = {'o': (fs2.from_cm(out.detach(), T).cpu(), o64, o32), 'dqkv': (fs2.from_cm(qc.grad, T).cpu(), d64, d32)}
    if qc.shape[2] > T:
        assert float(qc.grad[:, :, T:].abs().max()) == 0.0 and float(out.detach()[:, :, T:].abs().max()) == 0.0
    for name, (x, x64, x32) in got.items():
        err, allowed = OH.rel_err(x, x64), OH.yardstick(OH.rel_err(x32, x64), 1e-5)
        print(f'EDGE attention_bwd kind={kind} B={B} T={T} {name}: rel err {err:.2e}, allowed {allowed:.2e} (fp32 CPU {OH.rel_err(x32, x64):.2e})')
        assert bool(torch.isfinite(x).all())
        assert err <= allowed, (name, err, allowed)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------
LN_T = (1, 31, 32, 33, 70)
LN_B = 3


def _ln_input(kind, T, C, relu_in, g):
    if kind == 'plain':
        x = 2 * torch.randn(LN_B, T, C, generator=g) + 0.3
    elif kind == 'offset':                                          # large mean, small spread: E[x^2] - E[x]^2 would lose the variance
        x = 100 + 0.1 * torch.randn(LN_B, T, C, generator=g)
    elif kind == 'outlier':
        x = 2 * torch.randn(LN_B, T, C, generator=g) + 0.3
        x[:, :, 5] = 1e4
    else:
        assert kind == 'small'
        x = 1e-3 * torch.randn(LN_B, T, C, generator=g)
    if relu_in:                                                     # no ReLU input near zero
        x = torch.where(x < 0, -(x.abs() + 0.01), x.abs() + 0.01)
        assert float(x.abs().min()) >= 0.01
    return x


@pytest.mark.parametrize('kind', ['plain', 'offset', 'outlier', 'small'])
@pytest.mark.parametrize('C', [256, 248, 80, 8])
def test_layer_norm(C, kind):
    from diffsinger_amd import fs2
    g = torch.Generator().manual_seed(C + 11)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    worst, worst_ratio = 0.0, 0.0
    for T in LN_T:
        keep = OH.ragged_keep(LN_B, T)
        for relu_in in (False, True):
            x = _ln_input(kind, T, C, relu_in, g)
            xc = fs2.to_cm(x.to(DEV))
            r = F.relu(x) if relu_in else x
            for eps in (1e-5, 1e-12):
                y64 = F.layer_norm(r.double(), (C,), gamma.double(), beta.double(), eps)
                y32 = F.layer_norm(r, (C,), gamma, beta, eps)
                for kp in (None, keep):
                    w64, w32 = (y64, y32) if kp is None else (y64 * kp.double()[:, :, None], y32 * kp[:, :, None])
                    out = fs2.layer_norm_cm(xc, T, gd, bd, eps, relu_in=relu_in, keep=None if kp is None else kp.to(DEV).contiguous())
                    assert out.shape == xc.shape
                    if out.shape[2] > T:
                        assert float(out[:, :, T:].abs().max()) == 0.0
                    got = fs2.from_cm(out, T).cpu()
                    e32 = OH.rel_err(w32, w64)
                    err, allowed = OH.rel_err(got, w64), OH.yardstick(e32, 2e-6)
                    worst, worst_ratio = max(worst, err / allowed), max(worst_ratio, err / max(e32, 1e-300))
                    assert bool(torch.isfinite(got).all())
                    assert err <= allowed, (C, kind, T, relu_in, eps, kp is not None, err, allowed)
    print(f'EDGE layer_norm C={C} kind={kind}: uses at most {worst:.3f} of the allowed error; device / fp32-CPU error <= {worst_ratio:.2f}')


@pytest.mark.parametrize('C', [256, 80])
def test_layer_norm_of_all_zero_frames_is_beta(C):
    """All-zero frames, and frames the ReLU makes all-zero, give beta * keep bit for bit (mean 0, every deviation 0)."""
    from diffsinger_amd import fs2
    g = torch.Generator().manual_seed(C + 3)
    T = 33
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    keep = OH.ragged_keep(LN_B, T)
    x = torch.randn(LN_B, T, C, generator=g)
    x[0, 5:9] = 0
    x[1] = 0
    neg = -(torch.rand(LN_B, T, C, generator=g) + 0.01)              # relu_in makes these all-zero
    for xin, relu_in, rows in ((x, False, x.abs().sum(-1) == 0), (x, True, x.abs().sum(-1) == 0),
                               (torch.where((torch.arange(T) % 3 == 0)[None, :, None], neg, x), True, None)):
        if rows is None:
            rows = (torch.arange(T) % 3 == 0)[None, :].expand(LN_B, T) | (xin.abs().sum(-1) == 0)
        for eps in (1e-5, 1e-12):
            for kp in (None, keep):
                out = fs2.layer_norm_cm(fs2.to_cm(xin.to(DEV)), T, gamma.to(DEV), beta.to(DEV), eps, relu_in=relu_in,
                                        keep=None if kp is None else kp.to(DEV).contiguous())
                got = fs2.from_cm(out, T).cpu()
                want = beta[None, None, :].expand(LN_B, T, C) * (1 if kp is None else kp[:, :, None])
                assert int(rows.sum()) > 0 and torch.equal(got[rows], want[rows])
                assert float(out[:, :, T:].abs().max()) == 0.0


# ---- convolution -------------------------------------------------------------------------------------------------------------------------------
def _conv_device(a, T):
    """the device's channel-major output for the inputs of fs2_ops_helpers.conv_inputs; a dilation goes through the C ABI (dsf_conv1d_dilated)"""
    from diffsinger_amd import _lib, fs2
    xc = fs2.to_cm(a['x'].to(DEV))
    w, b = a['w'].to(DEV), a['b'].to(DEV)
    if a['dil'] == 1:
        return fs2.conv1d_cm(xc, T, w, fs2.PackedWeight(), b, scale=a['scale'], act=a['act'],
                             residual=None if a['res'] is None else fs2.to_cm(a['res'].to(DEV)),
                             keep=None if a['keep'] is None else a['keep'].to(DEV).contiguous())
    assert a['scale'] == 1.0 and a['act'] == 'none' and a['res'] is None and a['keep'] is None
    lib = _lib.load()
    Co, Ci, K = a['w'].shape
    out = torch.empty(xc.shape[0], Co, xc.shape[2], device=DEV, dtype=torch.float32)
    wp = fs2.PackedWeight().get(w)
    with torch.cuda.device(DEV):
        _lib.check(lib.dsf_conv1d_dilated(xc.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(), xc.shape[0], Ci, Co, K, a['dil'], T,
                                          torch.cuda.current_stream(DEV).cuda_stream), 'dsf_conv1d_dilated')
    return out


@pytest.mark.parametrize('case', OH.CONV_CASES, ids=lambda c: 'B{}T{}Ci{}Co{}K{}d{}'.format(*c[:6]))
def test_conv1d(case):
    from diffsinger_amd import fs2
    B, T, Ci, Co, K, dil, _ = case
    a = OH.conv_inputs(*case)
    y64, bnd = OH.conv64(a['x'], a['w'], a['b'], a['dil'], a['scale'], a['act'], a['res'], a['keep'])
    y32 = OH.conv_finish(OH.conv32(a['x'], a['w'], a['b'], a['dil']), a['scale'], a['act'], a['res'], a['keep'])
    e_cpu = float((y32.double() - y64).abs().max())
    outs = {}
    try:
        for mode in (0, 1):                                         # k_fs_conv, and k_fs_conv_ks wherever the shape allows it (Ci % 32 == 0)
            fs2.set_conv_split(mode)
            with torch.no_grad():
                out = _conv_device(a, T)
            assert out.shape == (B, Co, fs2.padded_frames(T))
            if out.shape[2] > T:
                assert float(out[:, :, T:].abs().max()) == 0.0
            got = outs[mode] = fs2.from_cm(out, T).cpu()
            share, e_dev = OH.used(got, y64, bnd), float((got.double() - y64).abs().max())
            print(f'EDGE conv {case[:6]} act={a["act"]} split={mode}: uses {share:.3f} of the bound; max err {e_dev:.2e}, '
                  f'device / fp32-CPU error {e_dev / max(e_cpu, 1e-300):.2f}')
            assert bool(torch.isfinite(got).all())
            assert share <= 1.0
    finally:
        fs2.set_conv_split(-1)
    if Ci % 32 == 0:
        assert bool(((outs[0].double() - outs[1].double()).abs() <= 2 * bnd).all())
    else:
        assert torch.equal(outs[0], outs[1])                        # no K-split form for this shape: the same kernel twice


@pytest.mark.parametrize('Ci,K,dil,names', [(256, 19, 1, ('K=19',)), (256, 4, 1, ('K=4',)), (12, 3, 1, ('Ci=12',)), (256, 3, 9, ('K=3', 'dil=9'))])
def test_conv1d_refuses_what_it_cannot_run(Ci, K, dil, names):
    """Through the C ABI: nonzero status, the message names the shape, nothing is launched (the output keeps its bits)."""
    from diffsinger_amd import _lib
    lib = _lib.load()
    B, T, Co, TS = 2, 33, 64, 64
    x = torch.zeros(B, max(Ci, 16), TS, device=DEV)
    wp = torch.zeros(1 << 20, device=DEV)                           # more than any of these shapes would read
    out = torch.full((B, Co, TS), 7.0, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        if dil == 1:
            rc = lib.dsf_conv1d(x.data_ptr(), wp.data_ptr(), None, out.data_ptr(), B, Ci, Co, K, T, 1.0, 0, None, None, stream)
        else:
            rc = lib.dsf_conv1d_dilated(x.data_ptr(), wp.data_ptr(), None, out.data_ptr(), B, Ci, Co, K, dil, T, stream)
    msg = lib.dsd_last_error().decode()
    print(f'EDGE conv refusal Ci={Ci} K={K} dil={dil}: rc {rc}, "{msg}"')
    assert rc != 0
    assert all(n in msg for n in names), msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- layout ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [80, 256])
@pytest.mark.parametrize('T', [1, 33])
def test_layout_changes_on_a_strided_view(C, T):
    from diffsinger_amd import fs2
    g = torch.Generator().manual_seed(C + T)
    big = torch.randn(3, 2 * T + 1, C + 5, generator=g).to(DEV)
    view = big[:, 1::2, 3:3 + C]                                    # [3, T, C], no stride is the contiguous one
    assert view.shape == (3, T, C) and not view.is_contiguous()
    a, b = fs2.to_cm(view), fs2.to_cm(view.contiguous())
    TS = fs2.padded_frames(T)
    assert a.shape == (3, C, TS) and torch.equal(a, b)
    assert torch.equal(a[:, :, :T], view.transpose(1, 2)) and float(a[:, :, T:].abs().max()) == 0.0
    assert torch.equal(fs2.from_cm(a, T), view)
    fast = torch.randn(3, C, T + 2, generator=g).to(DEV).transpose(1, 2)[:, 1:1 + T]      # frame axis fastest
    assert fast.shape == (3, T, C) and fast.stride(1) == 1
    assert torch.equal(fs2.to_cm(fast), fs2.to_cm(fast.contiguous())) and torch.equal(fs2.from_cm(fs2.to_cm(fast), T), fast)


# ---- one whole model at the benchmark's length --------------------------------------------------------------------------------------------------
def _long_case():
    import diffsinger_amd
    from diffsinger_amd import fs2, hparams
    from oracle.fs2_cases import VOCAB, make_inputs, synth_params
    hparams.clear()
    diffsinger_amd.use_preset('lj_ds_beta6')
    m = fs2.FastSpeech2(VOCAB, 80).eval()
    params = synth_params(FH.shapes_of(m), 1301)
    m.load_state_dict(params, strict=True)
    inp = make_inputs(dict(mode='teacher', B=2, T_txt=300, seed=301), False)
    return m, dict(hparams), params, inp


def test_fs2_forward_at_the_mel_rate_of_the_benchmark():
    """FastSpeech2 (lj_ds_beta6), 2 x 300 phones -> about 1050 frames, against the CPU oracle as test_fs2_matches_reference compares with its
    fixtures: mel2ph exact, decoder_inp / mel_out / the predictor outputs within the whole-model tolerance of 1e-4."""
    from oracle import fs2_oracle as FO
    m, hp, params, inp = _long_case()
    assert inp['mel2ph'].shape[1] > 1024
    kw = {k: v.clone() for k, v in inp.items() if k != 'txt_tokens'}
    with torch.no_grad():
        want = FO.fs2_forward(FH.oracle_params(params), hp, inp['txt_tokens'], **kw)
    md = m.to(DEV)
    with torch.no_grad():
        got = md(inp['txt_tokens'].to(DEV), infer=True, **{k: v.to(DEV) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert torch.equal(got['mel2ph'].cpu(), want['mel2ph'])
    seen = []
    for k in ('dur', 'pitch_pred', 'cwt', 'energy_pred', 'decoder_inp', 'mel_out'):
        if k not in want or not isinstance(want[k], torch.Tensor):
            continue
        assert k in got and got[k].shape == want[k].shape, k
        err = float((got[k].cpu() - want[k]).abs().max())
        print(f'EDGE fs2 {inp["mel2ph"].shape[1]} frames {k}: max-abs err {err:.3e} (max|ref| {float(want[k].abs().max()):.2f})')
        seen.append((k, err))
    assert {'decoder_inp', 'mel_out'} <= {k for k, _ in seen}
    assert all(e <= 1e-4 for _, e in seen), seen
