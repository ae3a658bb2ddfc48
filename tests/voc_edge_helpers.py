"""Test infrastructure of the vocoder's inference kernels (include/dsv.h: dsv_conv1d, dsv_conv1d_folded, dsv_noise_conv, dsv_pwg_layer,
dsv_pwg_upsample, dsv_pwg_first) at short lengths, workgroup and channel-slab seams and odd phase counts: float64 restatements on the CPU with
element-wise error bounds, the case tables of tests/test_gpu_voc_edges.py, and restated bugs ("mutants") that tests/test_voc_edges_host.py
applies inside the float64 model to prove that the bound catches them.  Plain torch on the CPU; only the weight transform `polyphase_weight`
(host code, checked against F.conv_transpose1d by the host test) comes from diffsinger_amd.

THE RULE (tests/pwg_disc_helpers.py, fs2_ops_helpers.py, pwg_train_helpers.py).  U = 2^-24; an fp32 sum of products may differ from float64 by
at most RULE = 16 U times the same sum over absolute values.  Every restatement takes the device's own float32 operands, converted to float64,
and returns (want, bound) on the padded sample axis: want is 0 and bound is 0 on [L, LS), so "within bound" there means exactly 0.

CONVOLUTION (conv64).  The header formula of dsv_conv1d: leaky ReLU in front, the stride-1 convolution over (input channel, tap), the
interleave n = q * up + phase of the polyphase rows, bias, + res, sum_in +, / divide, tanh.
    bound = RULE (sum |w| |lrelu x| + |bias| + |res| + |sum_in|) / |divide|        (+ 4 U with tanh: tanh is 1-Lipschitz, 4 U for tanhf as
                                                                                    tests/test_gpu_hifigan_train.py grants it)
The contraction is written as the WALK of the kernel's tiles - workgroup spans of the sample axis with their staged halo, channel slabs, taps -
so that a bug of that walk can be restated inside it (MUTANTS); with the switches off the walk is the convolution (host test: equal to
F.conv1d / F.conv_transpose1d to 1e-12).  `instantiation` restates which build of k_voc_conv the host dispatch of csrc/voc_abi.hpp picks,
from that file's own arithmetic; the GPU tests never take a number from it other than which seam a case is about.

FOLDED FORM (fold64).  The same convolution: dsv_conv1d_folded must equal the plain convolution, not its own restatement.  fold64 adds the
map of the folded columns (column c stands for samples pos(c) + e dil, e < F) only to state that every sample is produced exactly once and
to carry the one mutant of that map.

THE PWG GATE (pwg_layer64).  a = W1 [x(t - d); x(t); x(t + d); c(t)] + b1 carries bound_a by the rule.  z = tanh(a_t) sigmoid(a_g):
|tanh'| <= 1, |sigmoid'| <= 1/4, |tanh| <= 1, 0 < sigmoid < 1, so the first contraction's error moves z by at most bound_a_t + bound_a_g / 4.
On top of that the device's own evaluation of the gate gets the ABSOLUTE allowance GATE = RULE = 16 U, by this count (|z| <= 1):
  * __expf(v) is the 1-ulp hardware exp2 behind the product v log2(e).  Rounding that product moves the exponent's argument by at most
    U |v log2 e|, i.e. E = e^v by the factor (1 + U |v|) (ln 2 log2 e = 1); with the exp2's own ulp, E (1 + (|v| + 2) U).
  * tanh(a) = 1 - 2 / (E + 1), E = e^(2a): d tanh / d ln E = (1 - tanh^2) / 2, so E's error moves it by (1 - tanh^2)(|a| + 1) U <= 1.5 U
    (|a| (1 - tanh^2 a) <= 0.45); the rounding of E + 1 by another (1 - tanh^2) U / 2, the division by U 2 / (E + 1) <= 2 U, the
    subtraction by U: <= 5 U.  At E = inf (a > 44) and E = 0 (a < -44, or flushed to 0 earlier) the form gives exactly +1 and -1.
  * sigmoid(g) = 1 / (1 + E), E = e^-g: sigmoid (1 - sigmoid)(|g| + 2) U <= 0.8 U for E, U / 4 for 1 + E, U for the division: <= 2 U;
    exactly 1 and 0 at E = 0 and E = inf.
  * the product of the two: 5 U + 2 U + U = 8 U <= GATE.
The second contraction adds |W2| bound_z + RULE (|W2| |z| + |b2|); `+ x` and `* sqrt(0.5)` (sqrtf(0.5f), one rounding off sqrt(0.5)) add
4 U (|o| + |x|) sqrt(0.5), the running skip sum 2 U (|prev| + |o|)."""
import math

import torch
import torch.nn.functional as F

from diffsinger_amd.vocoder import polyphase_weight

U = 2.0 ** -24
RULE = 16.0 * U
GATE = RULE
S = math.sqrt(0.5)
HALO, HALO_WIDE, HALO_LEAN = 28, 48, 4           # kVocHalo, kVocHaloWide, kVocHaloLean of csrc/voc_kernels.hpp
LDS_BUDGET = 72 * 1024
FOLD_COLS = 256                                  # kFoldCols


def padded(L):
    return (L + 31) // 32 * 32


def d64(t):
    return None if t is None else t.detach().to('cpu', torch.float64)


def cm(x, L=None):
    """[B][C][L] -> [B][C][LS] with a zero tail (the device layout)"""
    L = x.shape[2] if L is None else L
    out = torch.zeros(x.shape[0], x.shape[1], padded(L), dtype=x.dtype)
    out[:, :, :L] = x[:, :, :L]
    return out


def used(got, want, bound):
    """largest |got - want| / bound over the elements; where the bound is 0 the value must be exactly `want`"""
    err = (d64(got) - want).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float('inf')
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


# ---- which build of k_voc_conv runs a shape (csrc/voc_abi.hpp dsv_conv1d, csrc/voc_kernels.hpp voc_span / voc_slab) ---------------------------
def span_of(nb, wt):
    return 32 * nb * wt


def slab_of(nb, wt, halo):
    return min(256, LDS_BUDGET // ((span_of(nb, wt) + 2 * halo) * 4) // 8 * 8)


def tall_workgroups(B, rows, L):
    return ((padded(L) + 127) // 128) * B * ((rows + 127) // 128)


def instantiation(B, ci, rows, k, pad, dil, L, up, lean=True):
    """(name, span, slab, halo) of the instantiation dsv_conv1d launches"""
    right = (k - 1) * dil - pad
    wide = pad > HALO or right > HALO
    if not wide and rows > 64 and tall_workgroups(B, rows, L) >= 512:
        nb, wt, halo, name = 4, 1, HALO, '<4,1>'
    elif rows <= 32:
        nb, wt, halo, name = 4, 4, HALO_WIDE if wide else HALO, '<4,4>'
        ci8 = (ci + 7) // 8 * 8
        if (not wide and up == 2 and lean and pad <= HALO_LEAN and right <= HALO_LEAN and ci8 <= slab_of(2, 4, HALO_LEAN)
                and ci8 * (span_of(2, 4) + 2 * HALO_LEAN) * 4 <= 40 * 1024):
            nb, wt, halo, name = 2, 4, HALO_LEAN, 'lean<2,4>'
    elif rows <= 64:
        nb, wt, halo, name = 2, 2, HALO_WIDE if wide else HALO, '<2,2>'
    else:
        nb, wt, halo, name = 1, 1, HALO_WIDE if wide else HALO, '<1,1>'
    return name + ('wide' if halo == HALO_WIDE else ''), span_of(nb, wt), slab_of(nb, wt, halo), halo


SLABS = {'<4,4>': 32, '<2,2>': 96, '<1,1>': 208, '<4,4>wide': 24, '<2,2>wide': 80, '<1,1>wide': 144, '<4,1>': 96}
SPANS = {'<4,4>': 512, '<2,2>': 128, '<1,1>': 32, '<4,4>wide': 512, '<2,2>wide': 128, '<1,1>wide': 32, '<4,1>': 128, 'lean<2,4>': 256}


# ---- dsv_conv1d ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ('halo', 'slab', 'phase', 'tail')


def mutant_seen(name, geom, ci, rows, L, up):
    """can the restated bug change any output of this case?"""
    _, span, slab, _ = geom
    if name == 'halo':            # (a) the left halo of every workgroup span after the first reads zero
        return L > span
    if name == 'slab':            # (b) the channels of a remainder slab are dropped
        return ci > slab and ci % slab != 0
    if name == 'phase':           # (c) at up > 1 the phase of the last, partial 32-row block is written one sample late
        return up > 1 and rows % 32 != 0
    if name == 'tail':            # (d) samples [L, LS) of the output keep their value before masking
        return padded(L * up) > L * up
    raise KeyError(name)


def _walk(xa, w, pad, dil, geom, mutant=None):
    """y[b][row][q] = sum_ci sum_t w[row][ci][t] xa[b][ci][q + t dil - pad] on q < LS, as the kernel walks it: per workgroup span its staged
    window (halo either side, zero outside [0, LS)), per channel slab, per tap"""
    B, Ci, LS = xa.shape
    rows, _, K = w.shape
    _, span, slab, halo = geom
    assert 0 <= pad <= halo and 0 <= (K - 1) * dil - pad <= halo
    y = torch.zeros(B, rows, LS, dtype=torch.float64)
    for t0 in range(0, LS, span):
        n = min(span, LS - t0)
        win = torch.zeros(B, Ci, span + 2 * halo, dtype=torch.float64)
        lo, hi = max(0, t0 - halo), min(LS, t0 + span + halo)
        win[:, :, lo - (t0 - halo):hi - (t0 - halo)] = xa[:, :, lo:hi]
        if mutant == 'halo' and t0 > 0:
            win[:, :, :halo] = 0
        for c0 in range(0, Ci, slab):
            nc = min(slab, Ci - c0)
            if mutant == 'slab' and c0 > 0 and nc < slab:
                continue
            for t in range(K):
                off = halo + t * dil - pad
                y[:, :, t0:t0 + n] += torch.einsum('rc,bcl->brl', w[:, c0:c0 + nc, t], win[:, c0:c0 + nc, off:off + n])
    return y


def _interleave(y, up, LSo, late_from=None):
    """out[b][co][q up + phase] = y[b][co up + phase][q]; rows >= late_from land one sample late (mutant)"""
    B, rows, LS = y.shape
    co = torch.arange(rows) // up
    shift = torch.zeros(rows, dtype=torch.long) if late_from is None else (torch.arange(rows) >= late_from).long()
    n = torch.arange(LS)[None, :] * up + (torch.arange(rows) % up + shift)[:, None]
    out = torch.zeros(B, rows // up, LS * up + 1, dtype=torch.float64)
    out[:, co[:, None].expand(rows, LS), n] = y
    if out.shape[2] < LSo:
        out = F.pad(out, (0, LSo - out.shape[2]))
    return out[:, :, :LSo]


def lrelu64(x, slope):
    x = d64(x)
    return torch.where(x > 0, x, x * float(slope))


def contract64(x, w, pad, dil, up=1, slope=1.0, geom=None, mutant=None, magnitudes=True):
    """(sum, sum over absolute values) of the contraction, interleaved, on [B][Co][LSo].  x [B][Ci][L] fp32, w [rows][Ci][K] fp32 (the polyphase
    form for up > 1).  Cached by the tests across the fused neighbours of one shape."""
    B, Ci, L = x.shape
    rows = w.shape[0]
    LS, LSo = padded(L), padded(L * up)
    geom = geom or ('whole', LS, Ci, HALO_WIDE)
    xa = cm(lrelu64(x, slope), L)
    w64 = d64(w)
    late = 32 * ((rows + 31) // 32 - 1) if (mutant == 'phase' and up > 1 and rows % 32) else None
    y = _interleave(_walk(xa, w64, pad, dil, geom, mutant), up, LSo, late)
    ya = _interleave(_walk(xa.abs(), w64.abs(), pad, dil, ('whole', LS, Ci, HALO_WIDE)), up, LSo) if magnitudes else torch.zeros_like(y)
    return y, ya


def conv64(x, w, bias, pad, dil, up=1, slope=1.0, res=None, sum_in=None, divide=1.0, act=0, geom=None, mutant=None, core=None):
    """(want, bound) of dsv_conv1d on [B][Co][LSo]; res / sum_in [B][Co][Lo] (or padded) fp32"""
    B, Ci, L = x.shape
    Lo, LSo = L * up, padded(L * up)
    y, ya = core if core is not None else contract64(x, w, pad, dil, up, slope, geom, mutant)
    v, a = y.clone(), ya.clone()
    if bias is not None:
        v = v + d64(bias)[None, :, None]
        a = a + d64(bias).abs()[None, :, None]
    if res is not None:
        r = cm(d64(res), Lo)
        v, a = v + r, a + r.abs()
    if sum_in is not None:
        s = cm(d64(sum_in), Lo)
        v, a = s + v, a + s.abs()
    dv = float(torch.tensor(divide, dtype=torch.float32))
    v, bound = v / dv, RULE * a / abs(dv)
    if act == 1:
        v, bound = torch.tanh(v), bound + 4 * U
    if mutant != 'tail':
        v[:, :, Lo:] = 0
    bound[:, :, Lo:] = 0
    return v, bound


FUSED = {                                        # every fused neighbour of the ABI
    'bare': dict(),
    'res': dict(res=True),
    'res+sum/3': dict(res=True, acc=True, div=3.0),
    'tanh': dict(slope=0.01, act=1),
    'all': dict(res=True, acc=True, div=3.0, slope=0.01, act=1),
}

# plain convolutions, B = 2: (tag, co, k, dil, Ci..., L...) - per instantiation one length below the reach of the taps, the workgroup span and one
# sample either side of it, a Ci one 8-group over the channel slab and one 4 over (nc8 > nc)
PLAIN = [
    ('<4,4>', 32, 11, 5, (8, 40, 36), (1, 24, 31, 32, 33, 511, 512, 513, 1049)),
    ('<2,2>', 64, 7, 5, (64, 104, 100), (1, 14, 127, 128, 129, 271)),
    ('<1,1>', 128, 7, 1, (128, 216, 212), (1, 2, 31, 32, 33, 67)),
    ('<4,4>wide', 32, 7, 12, (32, 28), (1, 35, 47, 48, 49, 511, 512, 513)),
    ('<4,4>wide', 32, 9, 12, (32, 28), (1, 35, 47, 48, 49, 511, 512, 513)),
    ('<2,2>wide', 64, 7, 12, (64, 88, 84), (1, 35, 47, 48, 49, 127, 128, 129)),
    ('<2,2>wide', 64, 9, 12, (64, 88, 84), (1, 35, 47, 48, 49, 127, 128, 129)),
    ('<1,1>wide', 128, 7, 12, (128, 152, 148), (1, 35, 47, 48, 49, 31, 32, 33)),
    ('<1,1>wide', 128, 9, 12, (128, 152, 148), (1, 35, 47, 48, 49, 31, 32, 33)),
]
SMALL_ROWS = [(co, 12, 5, 2, L) for co in (1, 5, 20) for L in (1, 31, 33, 513)]          # rows that fill no 32-row block
# transposed convolutions: (u, k, Co, Ci) - rows = Co u once below 32 and once in 33..64 with a partial last block
TRANSPOSED = [(2, 4, 5, 16), (2, 4, 21, 24), (3, 7, 5, 16), (3, 7, 11, 24), (4, 8, 5, 16), (4, 8, 11, 24), (5, 11, 5, 16), (5, 11, 9, 24),
              (6, 12, 5, 16), (6, 12, 7, 24), (8, 16, 3, 16), (8, 16, 5, 24)]
ODD_UP_HOST_LENGTHS = (1, 2, 31, 33)
# the tall build: (Ci, rows, K, up, B, L); K = 3 is the polyphase form of ConvTranspose1d(kernel 16, stride 8, padding 4)
TALL = [(8, 72, 3, 8, 128, 500), (104, 72, 3, 8, 128, 500), (100, 72, 3, 8, 128, 500)]
TALL_DISTINCT = 4
LEAN = [(16, 8), (32, 16), (8, 3)]               # (Ci, Co) of ConvTranspose1d(kernel 4, stride 2, padding 1)
LEAN_LENGTHS = (1, 31, 255, 256, 257, 513)


def transposed_geometry(u, k, co, ci, L, B=2, lean=True):
    w, pad = polyphase_weight(torch.zeros(ci, co, k), u, (k - u) // 2)
    return instantiation(B, ci, co * u, w.shape[2], pad, 1, L, u, lean)


def transposed_lengths(u, k, co, ci):
    span = transposed_geometry(u, k, co, ci, 64)[1]
    return (1, 2, 31, 32, 33, span - 1, span, span + 1)


def store_path(u):
    return '16-byte' if u % 4 == 0 else '8-byte' if u == 2 else 'general'


def seed_of(*key):
    s = 17
    for v in key:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def plain_case(co, ci, k, dil, L, B=2):
    """seeded operands of one plain convolution: x [B][Ci][L], w [co][Ci][k], bias, res, acc [B][co][L]"""
    g = torch.Generator().manual_seed(seed_of(co, ci, k, dil, L, B))
    return dict(x=torch.randn(B, ci, L, generator=g), w=torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5, bias=torch.randn(co, generator=g),
                res=torch.randn(B, co, L, generator=g), acc=torch.randn(B, co, L, generator=g), pad=(k - 1) * dil // 2, dil=dil, up=1, rows=co, L=L)


def transposed_case(u, k, co, ci, L, B=2, distinct=None):
    """seeded operands of ConvTranspose1d(ci -> co, kernel k, stride u, padding (k - u) / 2): `wt` the module's weight [Ci][Co][k], `w` / `pad`
    its polyphase form; `distinct`: the B utterances are that many different ones, repeated"""
    nb = distinct or B
    g = torch.Generator().manual_seed(seed_of(u, k, co, ci, L, nb))
    wt = torch.randn(ci, co, k, generator=g) / (ci * k / u) ** 0.5
    w, pad = polyphase_weight(wt, u, (k - u) // 2)
    rep = lambda t: t.repeat(B // nb, 1, 1) if distinct else t
    return dict(x=rep(torch.randn(nb, ci, L, generator=g)), wt=wt, w=w, bias=torch.randn(co, generator=g), res=rep(torch.randn(nb, co, L * u, generator=g)),
                acc=rep(torch.randn(nb, co, L * u, generator=g)), pad=pad, dil=1, up=u, rows=co * u, L=L)


def fused_kw(c, fused):
    """the keyword operands of conv64 / the header formula for one entry of FUSED"""
    f = FUSED[fused]
    return dict(slope=f.get('slope', 0.1), res=c['res'] if f.get('res') else None, sum_in=c['acc'] if f.get('acc') else None,
                divide=f.get('div', 1.0), act=f.get('act', 0))


# ---- dsv_conv1d_folded --------------------------------------------------------------------------------------------------------------------------
def fold_ld(F_):
    return 260 * F_ + 80


def fold_factor_model(co, ci, k, dil):
    """dsv_fold_factor of csrc/voc_abi.hpp restated (the GPU test asks the library and asserts that the two agree)"""
    if ci > 16 or not (k & 1):
        return 1
    F_ = 4 if co <= 8 else 2 if co <= 16 else 1
    if F_ == 1:
        return 1
    pad, KT = (k - 1) * dil // 2, k + F_ - 1
    maxcol = (254 + dil) * F_ + dil + 30 + (KT - 1) * dil - pad
    return F_ if (pad <= HALO - 3 and maxcol < fold_ld(F_)) else 1


def fold_max_dilation(co, ci, k):
    F_ = fold_factor_model(co, ci, k, 1)
    d = 1
    while fold_factor_model(co, ci, k, d + 1) == F_:
        d += 1
    return d


def fold_pos(c, F_, dil):
    return (c // dil) * F_ * dil + c % dil


FOLD_SHAPES = [(8, 8), (5, 12), (1, 8), (16, 16), (12, 12)]              # (Co, Ci): F = 4, 4, 4, 2, 2
FOLD_KERNELS = (3, 7, 11)


def fold_lengths(F_, dil):
    p = fold_pos(FOLD_COLS, F_, dil)
    return sorted({1, 2, 3, 5, F_ * dil - 1, F_ * dil, 31, 32, 33, p - 1, p, p + 1, p + F_ * dil + 1} - {0})   # the last: one whole group past the seam


def fold64(x, w, bias, F_, dil, mutant=None, **kw):
    """(want, bound) of dsv_conv1d_folded = of the plain 'same' convolution with the ORIGINAL weight w [co][ci][k].  The folded columns only
    decide which samples are written: every one exactly once; mutant 'column': column 256 takes the group of column 255."""
    L = x.shape[2]
    LS = padded(L)
    k = w.shape[2]
    want, bound = conv64(x, w, bias, (k - 1) * dil // 2, dil, 1, **kw)
    fd = F_ * dil
    groups = (LS + fd - 1) // fd
    hits = torch.zeros(groups * fd + fd, dtype=torch.long)
    for c in range(groups * dil):
        grp = c // dil
        if mutant == 'column' and c == FOLD_COLS:
            grp = (c - 1) // dil
        pos = grp * fd + (c - grp * dil)
        for e in range(F_):
            hits[pos + e * dil] += 1
    if mutant is None:
        assert bool((hits[:groups * fd] == 1).all()) and int(hits[groups * fd:].sum()) == 0
    want = torch.where((hits[:LS] > 0)[None, None, :], want, torch.zeros_like(want))
    return want, bound


def fold_mutant_seen(F_, dil, L):
    # the misplaced column still writes sample pos(256) (its last step); the first sample nobody writes is pos(256) + dil
    return FOLD_COLS % dil == 0 and fold_pos(FOLD_COLS, F_, dil) + dil < L


# ---- dsv_noise_conv -----------------------------------------------------------------------------------------------------------------------------
NOISE = [(64, 32, 64), (16, 2, 4), (8, 1, 1), (32, 6, 12)]               # (C, stride, K); pad = stride / 2, the generator's noise_convs (6: rates [5, 3, 2])


def noise_lengths(s):
    return (s, 2 * s, 33 * s, 8192 + s)


def noise_case(C, s, K, L_har, B=3):
    g = torch.Generator().manual_seed(seed_of(C, s, K, L_har))
    return dict(har=torch.tanh(torch.randn(B, L_har, generator=g)), w=torch.randn(C, K, generator=g) * 0.1, bias=torch.randn(C, generator=g), pad=s // 2,
                L_out=(L_har + 2 * (s // 2) - K) // s + 1)


def noise_conv64(har, w, bias, stride, pad, L_out):
    """out[b][c][n] = bias[c] + sum_j w[c][j] har[b][n s - pad + j] (zero outside [0, L_har)) -> (want, bound) on [B][C][LSo]"""
    B, Lh = har.shape
    C, K = w.shape
    i = torch.arange(L_out)[:, None] * stride - pad + torch.arange(K)[None, :]                     # [L_out][K]
    ok = ((i >= 0) & (i < Lh)).double()
    hg = d64(har)[:, i.clamp(0, Lh - 1)] * ok                                                      # [B][L_out][K]
    w64 = d64(w)
    y = torch.einsum('ck,bnk->bcn', w64, hg) + d64(bias)[None, :, None]
    ya = torch.einsum('ck,bnk->bcn', w64.abs(), hg.abs()) + d64(bias).abs()[None, :, None]
    return cm(y, L_out), cm(RULE * ya, L_out)


# ---- ParallelWaveGAN operators ------------------------------------------------------------------------------------------------------------------
PWG_LENGTHS = (1, 31, 32, 33, 64, 97)
PWG_DILATIONS = (1, 32, 512)
PWG_AUX = (0, 8, 80, 128)


def pwg_case(B, L, aux, scale=1.0, observe_gate=False):
    """seeded operands of one residual block; `scale` multiplies the gate pre-activations (weights and bias of the first contraction, with bias
    entries that reach +-120 when scale > 1); observe_gate: conv1x1_skip = identity without bias, so that with first = 1 the skip output IS z"""
    g = torch.Generator().manual_seed(seed_of(B, L, aux, int(scale), int(observe_gate)))
    K1 = 192 + aux
    c = dict(x=torch.randn(B, 64, L, generator=g), c=torch.randn(B, aux, L, generator=g) if aux else None,
             w1=torch.randn(128, K1, generator=g) * (2.0 * K1 ** -0.5) * scale, b1=torch.randn(128, generator=g) * 0.1 * scale,
             w2=torch.randn(128, 64, generator=g) * 0.125, b2=torch.randn(128, generator=g) * 0.1, prev=torch.randn(B, 64, L, generator=g))
    if scale > 1.0:
        c['b1'] = c['b1'] + torch.tensor([-120.0, -60.0, 0.0, 60.0, 120.0, 0.0, 25.0, -25.0]).repeat(16)
    if observe_gate:
        c['w2'][64:] = torch.eye(64)
        c['b2'][64:] = 0
    return c


def pwg_gate64(x, c, w1, b1, dil):
    """(tanh pre-activation, gate pre-activation, bound of either) [B][64][L] each, float64"""
    B, _, L = x.shape
    x64 = d64(x)
    xp = F.pad(x64, (dil, dil))
    rows = [xp[:, :, 0:L], xp[:, :, dil:dil + L], xp[:, :, 2 * dil:2 * dil + L]] + ([d64(c)] if c is not None else [])
    bt = torch.cat(rows, 1)                                                                        # [B][192 + aux][L]
    w, b = d64(w1), d64(b1)
    a = torch.einsum('rk,bkl->brl', w, bt) + b[None, :, None]
    ea = RULE * (torch.einsum('rk,bkl->brl', w.abs(), bt.abs()) + b.abs()[None, :, None])
    return a[:, :64], a[:, 64:], ea[:, :64], ea[:, 64:]


def pwg_layer64(x, c, w1, b1, w2, b2, dil, prev=None, gate_allowance=GATE):
    """k_pwg_layer's formula -> (x_out, bound, skip, bound, z) on [B][64][LS]; prev: the running skip sum coming in (None: first layer)"""
    L = x.shape[2]
    at, ag, et, eg = pwg_gate64(x, c, w1, b1, dil)
    z = torch.tanh(at) * torch.sigmoid(ag)
    ez = et + eg / 4 + gate_allowance
    w, b = d64(w2), d64(b2)
    o = torch.einsum('rk,bkl->brl', w, z) + b[None, :, None]
    eo = torch.einsum('rk,bkl->brl', w.abs(), ez) + RULE * (torch.einsum('rk,bkl->brl', w.abs(), z.abs()) + b.abs()[None, :, None])
    x64 = d64(x)
    xo = (o[:, :64] + x64) * S
    bx = (eo[:, :64] + 4 * U * (o[:, :64].abs() + x64.abs())) * S
    sk, bs = o[:, 64:], eo[:, 64:]
    if prev is not None:
        p = d64(prev)
        sk, bs = p + sk, bs + 2 * U * (p.abs() + o[:, 64:].abs())
    return cm(xo, L), cm(bx, L), cm(sk, L), cm(bs, L), z


def pwg_upsample64(x, w, scale):
    """out[r][t] = sum_j w[j] x[r][(t + j - scale) / scale] for 0 <= t + j - scale < L scale -> (want, bound) on [B][C][LSo]"""
    B, C, L = x.shape
    Lo = L * scale
    u = torch.arange(Lo)[:, None] + torch.arange(2 * scale + 1)[None, :] - scale                   # [Lo][2 scale + 1]
    ok = ((u >= 0) & (u < Lo)).double()
    xg = d64(x)[:, :, u.clamp(0, Lo - 1) // scale] * ok                                            # [B][C][Lo][taps]
    w64 = d64(w).reshape(-1)
    return cm(torch.einsum('bclj,j->bcl', xg, w64), Lo), cm(RULE * torch.einsum('bclj,j->bcl', xg.abs(), w64.abs()), Lo)


def pwg_first64(z, w, bias):
    """x[b][c][t] = w[c] z[b][t] + bias[c] -> (want, bound) on [B][C][LS]; z [B][L]"""
    L = z.shape[1]
    z64, w64, b64 = d64(z), d64(w), d64(bias)
    y = w64[None, :, None] * z64[:, None, :] + b64[None, :, None]
    ya = w64.abs()[None, :, None] * z64.abs()[:, None, :] + b64.abs()[None, :, None]
    return cm(y, L), cm(RULE * ya, L)
