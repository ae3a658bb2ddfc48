"""Test infrastructure of the FFT-block operators (include/dsf.h: dsf_attention, dsf_layer_norm, dsf_conv1d / dsf_conv1d_dilated) at the lengths and
score ranges the mel-rate decoder runs at: float64 restatements on the CPU with element-wise error CONDITIONS, the seeded inputs that drive the
attention core's online softmax into every branch, and a float32 emulation of that kernel's loop written from its comments
(csrc/fs2_kernels.hpp, k_fs_attn).  Plain torch on the CPU; nothing comes from diffsinger_amd.

THE RULE (tests/pwg_disc_helpers.py).  u = 2^-24; an fp32 sum of products may differ from float64 by at most RULE = 16 u times the same sum over
absolute values.

ATTENTION.  O = softmax(s) v with s_k = scale q.k.  A score error e_k moves the softmax-weighted sum, to first order, by
sum_k p_k e_k |v_k| + (sum_k p_k |v_k|) sum_k p_k e_k; the products P V and the normalisation add 2 RULE sum_k p_k |v_k|.  The score error is the
rule applied to the dot product plus the error of the exponential's argument, 4 u (|s_k - max s| + 6): the argument is formed in fp32 from
s log2 e and m log2 e, and the kernel's lazy reference maximum m may sit up to 5.5 below the true one (the 6).  Keys of probability 0 carry none.

CONVOLUTION.  y = (act(scale (W x + b)) + res) keep: the rule on the contraction through the activation's largest slope (1.13 bounds gelu, mish
and relu) plus 8 u (|act value| + |res|) for the activation's libm calls and the two additions.

YARDSTICK (tests/pe_train_helpers.py).  rel_err = max|X - X64| / max|X64|; allowed: max(4 x the fp32 CPU evaluation's rel_err, floor)."""
import math

import torch
import torch.nn.functional as F

from tests.pe_train_helpers import bound as _pe_bound
from tests.pe_train_helpers import rel_err  # noqa: F401  (re-exported: the tests take it from here)
from tests.pe_train_helpers import FLOOR as _PE_FLOOR

U = 2.0 ** -24
RULE = 16.0 * U
HD = 128
KINDS = ('flat', 'ramp_up_fast', 'ramp_up_slow', 'ramp_down', 'spike', 'offset')
SHAPES = ((1, 1), (2, 31), (2, 32), (3, 33), (3, 127), (3, 128), (3, 129), (3, 160), (3, 257), (3, 520), (1, 1030))
LOG2E = 1.4426950408889634
LAZY = 5.5


def seed_of(T):
    return 1000 + T


def yardstick(err32, floor):
    """allowed rel_err: max(4 x the fp32 CPU evaluation's, floor)"""
    assert floor >= _PE_FLOOR
    return max(_pe_bound(err32), float(floor))


def scale64():
    """head_dim ** -0.5 as the fp32 value the library multiplies q by ((float) sqrt(1 / 128)), in float64"""
    return float(torch.tensor(math.sqrt(1.0 / HD), dtype=torch.float32))


# ---- attention -------------------------------------------------------------------------------------------------------------------------------
def attention_inputs(kind, B, T, seed, heads=2):
    """(qkv [B, T, 3C] fp32, pad [B, T] bool).  Every kind but 'flat' adds sqrt(128) w to every head's q and beta[b, t] w to every head's k
    (w = ones(128) / sqrt(128)), so key t's score is about beta[b, t] above a key with beta 0, for every query."""
    if kind == 'spike' and T < 16:
        kind = 'flat'
    assert kind in KINDS
    C = HD * heads
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * C, generator=g)
    if kind != 'flat':
        w = torch.ones(HD) / math.sqrt(HD)
        tk = torch.arange(T, dtype=torch.float32)
        beta = torch.zeros(B, T)
        if kind == 'ramp_up_fast':
            beta[:] = 10.0 * tk / 128
        elif kind == 'ramp_up_slow':
            beta[:] = 3.0 * tk / 128
        elif kind == 'ramp_down':
            beta[:] = 10.0 * (T - 1 - tk) / 128
        elif kind == 'spike':
            for b in range(B):
                beta[b, [T - 7, 0, T // 2][b % 3]] = 30.0
        elif kind == 'offset':
            beta[:] = 100.0
        q = qkv[..., :C].view(B, T, heads, HD)
        k = qkv[..., C:2 * C].view(B, T, heads, HD)
        q += math.sqrt(HD) * w
        k += beta[:, :, None, None] * w
    pad = torch.zeros(B, T, dtype=torch.bool)
    for b in range(1, B):
        pad[b, max(1, T - 5 * b - 2):] = True
    if B > 1 and T > 96:
        pad[1, :64] = True                  # two leading key tiles dead: waves 0 and 1 start at m = -inf and go live later
    if B > 2 and T > 40:
        pad[2, 3] = pad[2, 37] = True       # padded keys inside live tiles
        if T > 200:
            pad[2, 130:170] = True          # a whole dead tile (128..159 holds 30 of them, 160..191 the rest) in the middle
    return qkv, pad


def _heads_of(qkv, heads, dtype):
    B, T, C3 = qkv.shape
    assert C3 == 3 * HD * heads
    return [t.reshape(B, T, heads, HD).transpose(1, 2) for t in qkv.to(dtype).chunk(3, -1)]


def attention_ref(qkv, pad, heads, dtype):
    """The torch restatement in `dtype` -> (O [B, T, C], s, p, q, k, v per head [B, heads, T, *])."""
    B, T, _ = qkv.shape
    q, k, v = _heads_of(qkv, heads, dtype)
    s = (q * torch.tensor(scale64(), dtype=dtype)) @ k.transpose(-1, -2)
    if pad is not None:
        s = s.masked_fill(pad[:, None, None, :], float('-inf'))
    p = torch.softmax(s, -1)
    o = (p @ v).transpose(1, 2).reshape(B, T, HD * heads)
    return o, s, p, q, k, v


def attention64(qkv, pad, heads):
    """(O, bound), both [B, T, C] float64."""
    B, T, _ = qkv.shape
    o, s, p, q, k, v = attention_ref(qkv, pad, heads, torch.float64)
    sabs = (q.abs() * scale64()) @ k.abs().transpose(-1, -2)
    m = s.max(-1, keepdim=True).values
    e = RULE * sabs + 4 * U * ((s - m).abs() + 6.0)
    e = torch.where(p > 0, e, torch.zeros_like(e))
    va = v.abs()
    pv = p @ va
    pe = p * e
    bnd = pe @ va + pv * pe.sum(-1, keepdim=True) + 2 * RULE * pv
    return o, bnd.transpose(1, 2).reshape(B, T, HD * heads)


def used(x, x64, bnd):
    """the largest share of the bound that |x - x64| uses, element-wise"""
    return float(((x.double() - x64).abs() / bnd.clamp_min(1e-300)).max())


def emulate_attention(qkv, pad, heads=2, lazy=LAZY, drop_rescale=False):
    """k_fs_attn's loop in fp32 on the CPU, from the kernel's comments: wave w of four takes the key tiles [32 w + 128 i, + 32) with its own
    (m, l, o); the reference maximum m is raised to the tile's maximum mx when mx > m + lazy or on the wave's first live tile, and only then l
    and o are multiplied by exp2((m_old - m_new) log2 e); P = exp2(s log2 e - m log2 e); the four partial results are merged by
    exp2((m_w - M) log2 e).  drop_rescale: the mutant that raises m without rescaling (alpha = 1).
    -> (O [B, T, C] fp32, raises after a wave's first live tile, number of P > 1)"""
    B, T, _ = qkv.shape
    q, k, v = [t.float() for t in _heads_of(qkv, heads, torch.float32)]
    q = q * torch.tensor(scale64(), dtype=torch.float32)
    l2e = torch.tensor(LOG2E, dtype=torch.float32)
    ninf = float('-inf')
    late_raises = above_one = 0
    ms, ls, os_ = [], [], []
    for w in range(4):
        m = torch.full((B, heads, T), ninf)
        l = torch.zeros(B, heads, T)
        o = torch.zeros(B, heads, T, HD)
        for tk0 in range(32 * w, T, 128):
            sl = slice(tk0, min(tk0 + 32, T))
            s = q @ k[:, :, sl].transpose(-1, -2)
            if pad is not None:
                s = s.masked_fill(pad[:, None, None, sl], ninf)
            mx = s.max(-1).values
            first = (m == ninf) & (mx > ninf)
            rz = (mx > m + lazy) | first
            late_raises += int((rz & ~first).sum())
            mn = torch.where(rz, mx, m)
            alpha = torch.where(m == ninf, torch.zeros_like(m), torch.exp2((m - mn) * l2e))
            if drop_rescale:
                alpha = torch.where(m == ninf, alpha, torch.ones_like(alpha))
            l, o, m = l * alpha, o * alpha[..., None], mn
            m2 = torch.where(m == ninf, torch.zeros_like(m), m * l2e)
            p = torch.exp2(s * l2e - m2[..., None])
            above_one += int((p > 1.0).sum())
            l = l + p.sum(-1)
            o = o + p @ v[:, :, sl]
        ms.append(m); ls.append(l); os_.append(o)
    M = torch.stack(ms).max(0).values
    sc = [torch.where(mw == ninf, torch.zeros_like(mw), torch.exp2((mw - M) * l2e)) for mw in ms]
    L = sum(l * c for l, c in zip(ls, sc))
    O = sum(o * c[..., None] for o, c in zip(os_, sc))
    inv = torch.where(L > 0, 1 / L, torch.zeros_like(L))
    return (O * inv[..., None]).transpose(1, 2).reshape(B, T, HD * heads), late_raises, above_one


# ---- convolution -----------------------------------------------------------------------------------------------------------------------------
# (B, T, Ci, Co, K, dil, extra): the full halo (K = 17; dil (K - 1) / 2 = 8), fewer frames than the reach, short second channel slabs
# (Ci = 264, 288), a long contraction with residual and mask, the narrowest operands, one frame, mish, gelu with a scale
CONV_CASES = (
    (2, 33, 256, 64, 17, 1, {}),
    (1, 8, 256, 257, 17, 1, {}),
    (2, 5, 256, 256, 3, 8, {}),
    (2, 40, 264, 65, 5, 2, {}),
    (2, 64, 288, 63, 9, 1, {}),
    (2, 77, 1024, 256, 1, 1, {'res': True, 'keep': True}),
    (2, 31, 8, 1, 3, 1, {}),
    (3, 1, 80, 128, 1, 1, {}),
    (2, 33, 256, 256, 1, 1, {'act': 'mish'}),
    (2, 33, 256, 1024, 9, 1, {'act': 'gelu', 'scale': 1.0 / 3.0}),
)


def ragged_keep(B, T):
    keep = torch.zeros(B, T)
    for b in range(B):
        keep[b, :T if b == 0 else max(1, T - 5 * b - 2)] = 1
    return keep


def conv_inputs(B, T, Ci, Co, K, dil, extra):
    """dict(x [B, T, Ci], w [Co, Ci, K], b [Co], res [B, T, Co] | None, keep [B, T] | None, dil, scale, act), seeded by the shape"""
    g = torch.Generator().manual_seed(B * 1000 + T + Ci + Co + K + 7 * dil)
    x = torch.randn(B, T, Ci, generator=g)
    w = torch.randn(Co, Ci, K, generator=g) * (Ci * K) ** -0.5
    b = torch.randn(Co, generator=g) * 0.1
    res = torch.randn(B, T, Co, generator=g) if extra.get('res') else None
    keep = ragged_keep(B, T) if extra.get('keep') else None
    return dict(x=x, w=w, b=b, res=res, keep=keep, dil=dil, scale=float(extra.get('scale', 1.0)), act=extra.get('act', 'none'))


def activation(v, act):
    if act == 'relu':
        return F.relu(v)
    if act == 'gelu':
        return F.gelu(v)
    if act == 'mish':
        return v * torch.tanh(F.softplus(v))
    assert act == 'none'
    return v


def _conv_btc(x, w, b, dil):
    K = w.shape[2]
    return F.conv1d(x.transpose(1, 2), w, b, padding=dil * (K - 1) // 2, dilation=dil).transpose(1, 2)


def conv_finish(pre, scale, act, res, keep):
    """(act(scale pre) + res) keep on [B, T, Co] in pre's dtype"""
    y = activation(pre * scale, act)
    if res is not None:
        y = y + res.to(y.dtype)
    if keep is not None:
        y = y * keep.to(y.dtype)[:, :, None]
    return y


def conv64(x, w, b, dil, scale, act, res, keep):
    """(y, bound), both [B, T, Co] float64; x [B, T, Ci], w [Co, Ci, K], b [Co] | None, res [B, T, Co] | None, keep [B, T] | None."""
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    a = activation(_conv_btc(x, w, b, dil) * scale, act)
    sabs = _conv_btc(x.abs(), w.abs(), None if b is None else b.abs(), dil)
    bnd = 1.13 * abs(scale) * RULE * sabs + 8 * U * a.abs()
    y = a
    if res is not None:
        y = y + res.double()
        bnd = bnd + 8 * U * res.double().abs()
    if keep is not None:
        y, bnd = y * keep.double()[:, :, None], bnd * keep.double()[:, :, None]
    return y, bnd


def conv_sabs64(x, w, b, dil):
    """sum |term| of the contraction in float64 (what RULE multiplies)"""
    return _conv_btc(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), dil)


def conv32(x, w, b, dil):
    """W x + b by aten's fp32 convolution"""
    return _conv_btc(x.float(), w.float(), None if b is None else b.float(), dil)


def conv32_sequential(x, w, b, dil):
    """W x + b as ONE strictly sequential fp32 chain over (ci, tap) per output: every product and every addition rounded once"""
    B, T, Ci = x.shape
    Co, _, K = w.shape
    half = dil * (K - 1) // 2
    xp = F.pad(x.float().transpose(1, 2), (half, half))                     # [B, Ci, T + 2 half]
    acc = torch.zeros(B, Co, T)
    for ci in range(Ci):
        for k in range(K):
            acc = acc + w[:, ci, k].float()[None, :, None] * xp[:, ci, k * dil:k * dil + T][:, None, :]
    if b is not None:
        acc = acc + b.float()[None, :, None]
    return acc.transpose(1, 2)
