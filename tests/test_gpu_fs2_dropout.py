"""GPU: FastSpeech2's counter-based training dropout (diffsinger_amd/dropout.py, csrc/fs2_dropout.hpp) against its host restatement
(tests/fs2_dropout_helpers.py, built on oracle/philox_oracle.py) - bit for bit: forward, backward, both memory paths, more than one pass of
the grid, every padding seam of the residual form; that no mask is saved; the advance() guard; one EncSALayer and a whole FastSpeech2 in
TRAIN mode (the first comparison of the train-mode forward and backward with anything), and that the switched-off path is the old one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffsinger_amd import _lib, dropout
from tests import fs2_dropout_helpers as DH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 1234


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    yield
    dropout.disable()


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------
# dropout_op
# ---------------------------------------------------------------------------------------------------------------
def _sizes():
    return [1, 3, 4, 5, 1023, 1024, 1025, int(_lib.load().dsf_dropout_grid_elements()) + 3]


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_op_equals_the_restated_mask_forward_and_backward(p):
    """Aligned buffers (float4 quads + the tail) and a view one element into its storage (one element per access), two sites, two steps."""
    st = dropout.DropoutState(DEV, SEED)
    assert _sizes()[-1] > 1025                                    # the last size needs more than one pass of the launch's grid
    for step in (0, 1):
        assert st.step == step
        for n in _sizes():
            x_h, dy_h = _rand(n + 1, n).numpy(), _rand(n, n + 7).numpy()
            for site in ((0, 5) if n <= 1025 else (1,)):
                for off in (0, 1):                                 # off = 1: the view x_store[1:], 4 bytes past a 16-byte boundary
                    store = torch.from_numpy(x_h).to(DEV)
                    x = store[off:off + n].detach().requires_grad_(True)
                    assert x.data_ptr() % 16 == 4 * off
                    y = dropout.dropout_op(x, p, st, site=site)
                    want = DH.dropout_ref(x_h[off:off + n], SEED, step, site, p)
                    assert _same_bits(y, want), (n, site, off, step)
                    y.backward(torch.from_numpy(dy_h).to(DEV))
                    assert _same_bits(x.grad, DH.dropout_ref(dy_h, SEED, step, site, p)), ('backward', n, site, off, step)
        st.advance()
    a, b = DH.kept(SEED, 0, 0, 1024, p), DH.kept(SEED, 1, 0, 1024, p)
    assert (a != b).any() and (a != DH.kept(SEED, 0, 5, 1024, p)).any()             # the cases above are different masks


def test_next_site_numbers_calls_in_execution_order():
    st = dropout.DropoutState(DEV, SEED)
    x_h = _rand(1000, 3).numpy()
    x = torch.from_numpy(x_h).to(DEV)
    for site in range(3):
        assert _same_bits(dropout.dropout_op(x, 0.5, st), DH.dropout_ref(x_h, SEED, 0, site, 0.5))
    st.advance()
    assert _same_bits(dropout.dropout_op(x, 0.5, st), DH.dropout_ref(x_h, SEED, 1, 0, 0.5))
    assert _same_bits(dropout.dropout_op(x, 0.5, st), DH.dropout_ref(x_h, SEED, 1, 1, 0.5))


# ---------------------------------------------------------------------------------------------------------------
# dropout_add_keep_op
# ---------------------------------------------------------------------------------------------------------------
def _ragged_keep(B, T):
    """Rows of different lengths; the last row of a batch of three is all padding."""
    lens = [T, (T + 1) // 2, 0][:B] if B > 1 else [(T + 1) // 2]
    keep = np.zeros((B, T), np.float32)
    for b, n in enumerate(lens):
        keep[b, :n] = 1
    return keep


@pytest.mark.parametrize('T', [1, 31, 32, 33, 95])
@pytest.mark.parametrize('C', [8, 256])
@pytest.mark.parametrize('B', [1, 3])
def test_dropout_add_keep_op_equals_the_restatement_in_y_dx_and_dres(B, C, T):
    TS = (T + 31) // 32 * 32
    st = dropout.DropoutState(DEV, SEED)
    x_h, r_h, dy_h = (_rand((B, C, TS), s + 100 * T + C + B).numpy() for s in (1, 2, 3))       # nonzero tails: they must not leak
    for keep_h, p, site in ((_ragged_keep(B, T), 0.1, 0), (None, 0.5, 3)):
        x, res = (torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (x_h, r_h))
        keep = torch.from_numpy(keep_h).to(DEV) if keep_h is not None else None
        y = dropout.dropout_add_keep_op(x, res, keep, T, p, st, site=site)
        assert _same_bits(y, DH.add_keep_ref(x_h, r_h, keep_h, T, SEED, 0, site, p)), ('y', keep_h is None)
        assert not _bits(y[:, :, T:]).any()                                                    # +0 bit patterns in [T, TS)
        y.backward(torch.from_numpy(dy_h).to(DEV))
        dx_w, dres_w = DH.add_keep_bwd_ref(dy_h, keep_h, T, SEED, 0, site, p)
        assert _same_bits(x.grad, dx_w), ('dx', keep_h is None)
        assert _same_bits(res.grad, dres_w), ('dres', keep_h is None)
        assert not _bits(x.grad[:, :, T:]).any() and not _bits(res.grad[:, :, T:]).any()
    # dres == NULL: a residual that needs no gradient
    x = torch.from_numpy(x_h).to(DEV).requires_grad_(True)
    dropout.dropout_add_keep_op(x, torch.from_numpy(r_h).to(DEV), None, T, 0.5, st, site=3).backward(torch.from_numpy(dy_h).to(DEV))
    assert _same_bits(x.grad, dx_w)

    # views one element into their storage: the one-element-per-access path of both kernels draws the mask of the views' own flat indices
    def off1(a):
        t = torch.cat([torch.zeros(1), torch.from_numpy(a).reshape(-1)]).to(DEV)[1:].view(B, C, TS)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    x, res = off1(x_h).requires_grad_(True), off1(r_h).requires_grad_(True)
    y = dropout.dropout_add_keep_op(x, res, None, T, 0.5, st, site=3)
    assert _same_bits(y, DH.add_keep_ref(x_h, r_h, None, T, SEED, 0, 3, 0.5))
    y.backward(off1(dy_h))
    assert _same_bits(x.grad, dx_w) and _same_bits(res.grad, dres_w)


# ---------------------------------------------------------------------------------------------------------------
# the autograd nodes
# ---------------------------------------------------------------------------------------------------------------
def test_neither_op_saves_a_tensor_of_the_activations_size():
    st = dropout.DropoutState(DEV, SEED)
    saved = []

    def pack(t):
        saved.append(t.numel())
        return t

    B, C, T = 2, 64, 40
    x, res = (_rand((B, C, 64), s).to(DEV).requires_grad_(True) for s in (1, 2))
    keep = torch.from_numpy(_ragged_keep(B, T)).to(DEV)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y1 = dropout.dropout_op(x, 0.1, st)
        y2 = dropout.dropout_add_keep_op(x, res, keep, T, 0.1, st)
        n_ours = list(saved)
        y3 = F.dropout(x, 0.1, True)                                # the hook sees torch's saved mask: the check can fail
    assert saved[len(n_ours):] and max(saved[len(n_ours):]) >= x.numel()
    assert all(n < x.numel() for n in n_ours), n_ours
    (y1.sum() + y2.sum() + y3.sum()).backward()


def test_advance_between_forward_and_backward_raises():
    st = dropout.DropoutState(DEV, SEED)
    x, res = (_rand((1, 8, 32), s).to(DEV).requires_grad_(True) for s in (1, 2))
    y1 = dropout.dropout_op(x, 0.5, st)
    y2 = dropout.dropout_add_keep_op(x, res, None, 20, 0.5, st)
    st.advance()
    with pytest.raises(RuntimeError, match='advance'):
        y1.sum().backward()
    with pytest.raises(RuntimeError, match='advance'):
        y2.sum().backward()
    y3 = dropout.dropout_op(x, 0.5, st)                             # a forward of the new step is fine
    y3.sum().backward()


# ---------------------------------------------------------------------------------------------------------------
# one EncSALayer in train mode
# ---------------------------------------------------------------------------------------------------------------
def _layer_case():
    from diffsinger_amd import fs2
    torch.manual_seed(11)
    C, B, T, p = 256, 2, 40, 0.1
    layer = fs2.EncSALayer(C, 2, kernel_size=9, dropout=p).to(DEV).train()
    with torch.no_grad():
        for prm in (layer.layer_norm1.weight, layer.layer_norm2.weight):
            prm.add_(0.1 * torch.randn_like(prm))
        for prm in (layer.layer_norm1.bias, layer.layer_norm2.bias, layer.ffn.ffn_2.bias):
            prm.add_(0.1 * torch.randn_like(prm))
    keep_h = np.zeros((B, T), np.float32)
    keep_h[0, :] = 1
    keep_h[1, :23] = 1
    keep = torch.from_numpy(keep_h).to(DEV)
    pad_u8 = (keep == 0).to(torch.uint8).contiguous()
    x0 = fs2.to_cm(_rand((B, T, C), 5).to(DEV) * keep[:, :, None])
    dy = _rand(tuple(x0.shape), 6).to(DEV)
    return fs2, layer, x0, dy, keep, pad_u8, T, p


def _composed_layer(fs2, layer, x, T, keep, pad_u8, drop):
    """EncSALayer.forward_cm in train mode from the existing operators; drop(site, t) applies that site's dropout as a torch expression."""
    a, f = layer.self_attn, layer.ffn
    kc = fs2._keep_cm(keep, x.shape[2])
    y = fs2.layer_norm_cm(x, T, layer.layer_norm1.weight, layer.layer_norm1.bias, 1e-5)
    qkv = fs2.conv1d_cm(y, T, a.in_proj_weight, a._pin)
    o = fs2.attention_cm(qkv, T, pad_u8, layer.num_heads)
    x = (x + drop(0, fs2.conv1d_cm(o, T, a.out_proj.weight, a._pout))) * kc
    y = fs2.layer_norm_cm(x, T, layer.layer_norm2.weight, layer.layer_norm2.bias, 1e-5, keep=None)
    hdn = fs2.conv1d_cm(y, T, f.ffn_1.weight, f._p1, f.ffn_1.bias, scale=f.kernel_size ** -0.5, act=f.act)
    out = fs2.conv1d_cm(drop(1, hdn), T, f.ffn_2.weight, f._p2, f.ffn_2.bias)
    return (x + drop(2, out)) * kc


def _grads(layer, x):
    g = {k: v.grad.clone() for k, v in layer.named_parameters()}
    g['input'] = x.grad.clone()
    layer.zero_grad(set_to_none=True)
    return g


def test_enc_sa_layer_in_train_mode_equals_its_composition_with_the_host_masks():
    fs2, layer, x0, dy, keep, pad_u8, T, p = _layer_case()
    scale = float(DH.scale_of(p))
    dropout.enable(SEED, DEV)
    x1 = x0.clone().requires_grad_(True)
    out1 = layer.forward_cm(x1, T, keep, pad_u8)
    assert dropout.current()._site == 3
    out1.backward(dy)
    g1 = _grads(layer, x1)
    dropout.disable()

    def drop(site, t):
        m = torch.from_numpy(DH.kept(SEED, 0, site, t.numel(), p).reshape(tuple(t.shape))).to(DEV)
        return torch.where(m, t * scale, torch.zeros((), device=DEV))

    x2 = x0.clone().requires_grad_(True)
    out2 = _composed_layer(fs2, layer, x2, T, keep, pad_u8, drop)
    out2.backward(dy)
    g2 = _grads(layer, x2)
    assert _same_bits(out1[:, :, :T], out2[:, :, :T])
    assert not _bits(out1[:, :, T:]).any() and float(out2.detach()[:, :, T:].abs().max()) == 0      # the fused op writes +0, the expression +-0
    assert float(out1.detach().abs().max()) > 0.1
    assert sorted(g1) == sorted(g2) and len(g1) >= 9
    for k in g1:                                                    # same kernels, same inputs: at most sums that arrive in another order
        err, top = float((g1[k] - g2[k]).abs().max()), float(g2[k].abs().max())
        print(f'{k}: max |g| {top:.3e}, max difference {err:.3e} = {err / max(top, 1e-30):.2e} of it')
        assert top > 0 and err <= 2.0 ** -22 * top, k


def test_switched_off_train_mode_is_the_old_code_path():
    """Feature off: EncSALayer and a predictor stack under torch.manual_seed(0) equal the former branches (F.dropout between the convolutions and
    the residual adds; the nn.Dropout module of the stack), called here as they stood."""
    fs2, layer, x0, dy, keep, pad_u8, T, p = _layer_case()
    assert dropout.current() is None
    with torch.no_grad():
        torch.manual_seed(0)
        got = layer.forward_cm(x0, T, keep, pad_u8)
        torch.manual_seed(0)
        want = _composed_layer(fs2, layer, x0, T, keep, pad_u8, lambda site, t: F.dropout(t, p, True))
        assert _same_bits(got, want)
        convs = fs2._pred_convs(256, 2, 256, 3, 0.5, 'SAME').to(DEV).train()
        packs = [fs2.PackedWeight() for _ in convs]
        torch.manual_seed(0)
        got = fs2._run_pred_convs(convs, packs, x0, T, keep)
        torch.manual_seed(0)
        xc = x0
        for seq, pk in zip(convs, packs):
            xc = fs2.layer_norm_cm(fs2.conv1d_cm(xc, T, seq[1].weight, pk, seq[1].bias), T, seq[3].weight, seq[3].bias, 1e-12, relu_in=True, keep=keep)
            xc = seq[4](xc)
        assert _same_bits(got, xc) and float((got == 0).float().mean()) > 0.4


# ---------------------------------------------------------------------------------------------------------------
# FastSpeech2 in train mode
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fs2_case():
    from oracle.check_fs2_grad import loss_of
    from tests import fs2_helpers as FH
    name = 'fs2_lj_teacher'
    case, m, hp, params, inp = FH.case_setup(name)
    assert hp['dropout'] == 0.1 and hp['predictor_dropout'] == 0.5
    m = m.to(DEV)
    tok = inp['txt_tokens'].to(DEV)
    kw = {k: v.clone().to(DEV) for k, v in inp.items() if k != 'txt_tokens'}

    def run(train=True, backward=True):
        m.train(train)
        m.zero_grad(set_to_none=True)
        r = m(tok, skip_decoder=True, infer=False, **{k: v.clone() for k, v in kw.items()})
        out = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v) and v.is_floating_point()}
        grads = {}
        if backward:
            loss_of(r, case['seed']).backward()
            grads = {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None}
        return out, grads

    return run


def _all_same(a, b):
    return sorted(a) == sorted(b) and all(_same_bits(a[k], b[k]) for k in a)


def test_fastspeech2_train_mode_is_reproducible_from_seed_and_step(fs2_case):
    """Deterministic algorithms are asked of torch for the glue that is not ours (the backward of the length regulator's torch.gather adds with
    atomics otherwise): what is checked is that the dropout - every site of it - is a function of (seed, step)."""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        dropout.enable(SEED, DEV)
        out_a, g_a = fs2_case()
        sites = dropout.current()._site
        st = dropout.enable(SEED, DEV)
        out_b, g_b = fs2_case()
        assert sites >= 15 and len(g_a) >= 60 and 'decoder_inp' in out_a
        assert _all_same(out_a, out_b) and _all_same(g_a, g_b)
        st.advance()
        out_c, g_c = fs2_case()
        assert not _same_bits(out_a['decoder_inp'], out_c['decoder_inp'])
        assert any(not _same_bits(g_a[k], g_c[k]) for k in g_a)
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])


def test_fastspeech2_eval_mode_does_not_see_the_switch(fs2_case):
    with torch.no_grad():
        off, _ = fs2_case(train=False, backward=False)
        st = dropout.enable(SEED, DEV)
        on, _ = fs2_case(train=False, backward=False)
        assert st._site == 0                                        # nothing consulted the state
    assert _all_same(off, on)


def test_fastspeech2_switched_off_train_mode_draws_from_torchs_generator_as_before(fs2_case):
    with torch.no_grad():
        torch.manual_seed(0)
        a, _ = fs2_case(backward=False)
        dropout.enable(SEED, DEV)
        dropout.disable()                                           # a switch that was on leaves nothing behind
        torch.manual_seed(0)
        b, _ = fs2_case(backward=False)
        torch.manual_seed(1)
        c, _ = fs2_case(backward=False)
    assert _all_same(a, b) and not _same_bits(a['decoder_inp'], c['decoder_inp'])
