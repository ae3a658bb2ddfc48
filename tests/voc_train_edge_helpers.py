"""Test infrastructure of the vocoder's TRAINING kernels (csrc/hifigan_train.hpp, pwg_train.hpp, voc_train_common.hpp behind hifigan_train_abi.hpp
and pwg_train_abi.hpp) at every tiling, slab count, clamp and split seam the C ABI admits: the case tables of tests/test_gpu_voc_train_edges.py,
a restatement of dsv_hgt_conv_dgrad's host dispatch, seeded operands and the float64 references with their element-wise bounds.  Plain torch on
the CPU.  tests/test_voc_train_edges_host.py asserts that the tables hold the paths they claim and runs every reference once on the CPU.

Nothing is re-chosen here.  The rule (RULE = 16 U, U = 2^-24, E_GATE, GATE_RANGE) is tests/pwg_train_helpers.py's; the references are
hifigan_train_helpers.conv_dgrad / conv_wgrad / conv_transpose_backward / noise_conv_backward and pwg_train_helpers.gate_backward /
conv_backward / wgrad_conv / wgrad_out / wgrad_relu; slab_of / span_of / SLABS / SPANS are tests/voc_edge_helpers.py's (k_hgt_dgrad stages and
tiles as k_voc_conv does, with the same constants).

THE DISPATCH (dgrad_dispatch; csrc/hifigan_train_abi.hpp dsv_hgt_conv_dgrad).  C <= 32 output rows take the <4,4> build (one 32-row block per
workgroup, span 512), anything wider the <2,2> build (two 32-row blocks per workgroup, span 128).  The build is the wide one (halo 48) when the
forward padding or the flipped padding (K - 1) dil - pad exceeds 28.  Cg, the channels of the incoming gradient, are cut into slabs of
32 / 96 / 24 / 80 channels; a last slab that is no multiple of 8 is staged with zero rows up to the next multiple.  On <2,2> an odd number of
32-row blocks leaves the last workgroup's second wave pair without a block: those waves are CLAMPED to the last block, walk its weights and
store nothing.

THE TABLES.  A length given as (a, b) stands for a * S + b samples, S the weight gradient's split length (dsv_hgt_wgrad_split(), kSplitK).
TABLE NOISE: the row (30, [(4, 15, 30)]) gives L_out = (30 + 14 - 30) // 15 + 1 = 1, not 2; it is kept as written (a second L_out = 1 case, at
stride 15) and (31, [(4, 15, 30)]), the shortest signal with two outputs at that stride, stands beside it."""
import os
import re

import torch
import torch.nn.functional as F

from tests import hifigan_train_helpers as TH
from tests import pwg_train_helpers as PH
from tests import voc_edge_helpers as E

RULE, U, E_GATE, GATE_RANGE = PH.RULE, PH.U, PH.E_GATE, PH.GATE_RANGE
GUARD = 64                                       # NaN floats either side of every output buffer (tests/test_gpu_hifigan_mpd.py's guard)
SLOPE = TH.LRELU_SLOPE
SUM_CHUNK = 1024                                 # kHgtSumChunk of csrc/hifigan_train.hpp
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffsinger_amd', 'csrc')


def header_constant(header, name):
    """`constexpr int <name> = <product of integers>;` parsed from the header's text"""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r'constexpr\s+int\s+' + re.escape(name) + r'\s*=\s*([0-9][0-9\s*]*);', f.read())
    assert m, f'{name} is not a constant of {header}'
    v = 1
    for factor in m.group(1).split('*'):
        v *= int(factor)
    return v


def length(spec, S):
    return spec if isinstance(spec, int) else spec[0] * S + spec[1]


def seed_of(*key):
    return E.seed_of(*[int(v) for v in key])


def rnd(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def cut(t, L):
    """a padded device tensor (or None) as unpadded float64 on the CPU"""
    return None if t is None else TH.d64(t)[..., :L]


def taps_of(k, u):
    """ConvTranspose1d(kernel k, stride u, padding (k - u) / 2) as polyphase rows: per tap its phase and its column in the polyphase filter, the
    polyphase kernel size and its padding (tests/test_gpu_hifigan_train.py's taps_of; the host test asserts that the two agree)"""
    p = (k - u) // 2
    r = [(j - p) % u for j in range(k)]
    dlt = [(r[j] + p - j) // u for j in range(k)]
    return r, [v - min(dlt) for v in dlt], max(dlt) - min(dlt) + 1, -min(dlt)


# ---- dsv_hgt_conv_dgrad's dispatch ----------------------------------------------------------------------------------------------------------------
BUILDS = {'<4,4>': (4, 4, E.HALO), '<2,2>': (2, 2, E.HALO), '<4,4>wide': (4, 4, E.HALO_WIDE), '<2,2>wide': (2, 2, E.HALO_WIDE)}


def dgrad_dispatch(C, Cg, K, dil, pad):
    """-> dict(tag, span, slab, slabs: the slab sizes Cg is cut into, blocks: 32-row blocks of C, z: workgroups along the rows, clamped: a wave
    without a block of its own, reach: the larger of the two paddings)"""
    flipped = (K - 1) * dil - pad
    assert 1 <= C <= 1024 and 1 <= Cg <= 1024 and 0 <= pad <= E.HALO_WIDE and 0 <= flipped <= E.HALO_WIDE, 'the ABI refuses this shape'
    wide = pad > E.HALO or flipped > E.HALO
    tag = ('<4,4>' if C <= 32 else '<2,2>') + ('wide' if wide else '')
    nb, wt, halo = BUILDS[tag]
    slab, wr = E.slab_of(nb, wt, halo), 4 // wt
    blocks, z = (C + 31) // 32, (C + 32 * wr - 1) // (32 * wr)
    return dict(tag=tag, span=E.span_of(nb, wt), slab=slab, slabs=[min(slab, Cg - c0) for c0 in range(0, Cg, slab)], blocks=blocks, z=z,
                clamped=z * wr > blocks, reach=max(pad, flipped), wide_by=(pad > E.HALO, flipped > E.HALO))


# ---- TABLE DGRAD: (tag, C, Cg, K, dil, pad) ---------------------------------------------------------------------------------------------------------
def _same(K, dil):
    return (K - 1) * dil // 2


DGRAD = ([('<4,4>', 32, cg, 11, 5, 25) for cg in (32, 40, 36)]                                                   # one slab, 32 + 8, 32 + 4
         + [('<4,4>wide', 32, cg, k, 12, _same(k, 12)) for k in (7, 9) for cg in (24, 32, 28)]                   # reach 36 and 48: one slab, 24 + 8, 24 + 4
         + [('<2,2>', c, cg, 11, 5, 25) for c, cg in ((40, 40), (72, 72), (64, 100), (64, 192), (256, 256))]     # .., clamp, 96 + 4, 96 + 96, 96 + 96 + 64
         + [('<2,2>wide', c, cg, k, 12, _same(k, 12)) for k in (7, 9) for c, cg in ((64, 64), (64, 88), (64, 84), (72, 72), (128, 128))]
         + [('<4,4>', 16, 16, 3, 1, 0), ('<4,4>', 16, 16, 4, 3, 2),                                             # asymmetric padding
            ('<2,2>wide', 64, 64, 5, 12, 8), ('<2,2>wide', 64, 64, 5, 12, 40)])                                  # wide through the flipped / the forward side only
WIDE_SHORT = (35, 47, 48, 49)                    # below, at and just above the wide builds' reach


def dgrad_cases():
    """(tag, C, Cg, K, dil, pad, B, L, form, masked): every row at B = 2, L = SPAN + 1; the first row of each instantiation also at
    L = 1, SPAN - 1, SPAN (and 35, 47, 48, 49 on the wide builds) with B = 1, in `second` form and with x_saved = nullptr"""
    out, seen = [], set()
    for row in DGRAD:
        tag = row[0]
        span = E.SPANS[tag]
        out.append(row + (2, span + 1, 'first', True))
        if tag not in seen:
            seen.add(tag)
            for L in (1, span - 1, span) + (WIDE_SHORT if tag.endswith('wide') else ()):
                out.append(row + (1, L, 'first', True))
            out += [row + (2, span + 1, 'second', True), row + (2, span + 1, 'first', False)]
    return out


def dgrad_id(case):
    tag, C, Cg, K, dil, pad, B, L, form, masked = case
    return f'{tag}-C{C}-Cg{Cg}-k{K}d{dil}p{pad}-B{B}-L{L}-{form}{"" if masked else "-nomask"}'


DGRAD_REPEAT = ('<2,2>', 256, 256, 11, 5, 25, 2, 129, 'first', True)        # three slabs, four workgroups along the rows


def dgrad_operands(case):
    """seeded float32 operands: g [B][Cg][L], w [Cg][C][K] (the forward convolution's weight, C -> Cg), x [B][C][L], res / sum_in or None"""
    tag, C, Cg, K, dil, pad, B, L, form, masked = case
    seed = seed_of(C, Cg, K, dil, pad, B, L)
    second = form == 'second'
    return dict(w=rnd(Cg, C, K, seed=seed) * (C * K) ** -0.5, g=rnd(B, Cg, L, seed=seed + 1), x=rnd(B, C, L, seed=seed + 2),
                res=rnd(B, C, L, seed=seed + 3) if second else None, sum_in=rnd(B, C, L, seed=seed + 4) if second else None,
                divide=3.0 if second else 1.0)


def dgrad_reference(case, g, w, x, res, sum_in):
    """float64 operands, unpadded -> {'dx', 'dw' [Cg][C][K], 'db'}: (want, bound)"""
    tag, C, Cg, K, dil, pad, B, L, form, masked = case
    dx = TH.conv_dgrad(g, w, x if masked else None, dil, pad, SLOPE, res, sum_in, 3.0 if form == 'second' else 1.0)
    dw, db = TH.conv_wgrad(g, x, K, dil, pad, SLOPE)
    return dict(dx=dx, dw=dw, db=db)


def tap_meets_signal(K, dil, pad, L):
    """[K] bool: tap k of a convolution reads at least one sample of [0, L) for some output of [0, L)"""
    return torch.tensor([abs(k * dil - pad) < L for k in range(K)])


# ---- TABLE WGRAD ----------------------------------------------------------------------------------------------------------------------------------
WGRAD_UP = [(2, 16, 8, 2, 4, (1, 1)), (1, 32, 16, 4, 8, (2, 37)),           # (B, Ci, Co, u, k, L): transposed, crossing a split
            (1, 16, 24, 8, 16, 33)]                                          # 192 rows: the second 128-row block has two dead waves
WGRAD_PLAIN = [(2, 8, 8, 3, (4, 0)), (3, 8, 8, 3, (3, 5)), (3, 8, 8, 3, (5, 0))]     # (B, Ci, Co, K, L), dilation 1, padding 1: 8, 12, 15 splits
WGRAD_BITS = (3, 64, (3, 5))                     # (B, channels, L) of the bit-equality of dsv_pwgt_wgrad_relu and dsv_hgt_conv_wgrad: 12 splits
WGRAD_REPEAT = ('plain', 1)


def splits_of(B, L, S):
    return B * ((L + S - 1) // S)


def wgrad_cases():
    return [('up', i) for i in range(len(WGRAD_UP))] + [('plain', i) for i in range(len(WGRAD_PLAIN))]


def wgrad_operands(kind, i, S):
    if kind == 'up':
        B, Ci, Co, u, k, L = WGRAD_UP[i]
        L = length(L, S)
        seed = seed_of(B, Ci, Co, u, k, L)
        return dict(B=B, Ci=Ci, Co=Co, u=u, k=k, L=L, g=rnd(B, Co, L * u, seed=seed + 1), x=rnd(B, Ci, L, seed=seed + 2))
    B, Ci, Co, K, L = WGRAD_PLAIN[i]
    L = length(L, S)
    seed = seed_of(B, Ci, Co, K, L)
    return dict(B=B, Ci=Ci, Co=Co, u=1, k=K, L=L, g=rnd(B, Co, L, seed=seed + 1), x=rnd(B, Ci, L, seed=seed + 2))


def wgrad_reference(c, g, x):
    """-> (want, bound) in the plain weight's layout: [Ci][Co][k] transposed, [Co][Ci][K] plain"""
    if c['u'] > 1:
        return TH.conv_transpose_backward(g, x, torch.zeros(c['Ci'], c['Co'], c['k'], dtype=torch.float64), c['u'], SLOPE)[1]
    return TH.conv_wgrad(g, x, c['k'], 1, 1, SLOPE)[0]


# ---- TABLE ROWSUM: (B, C, L) ------------------------------------------------------------------------------------------------------------------------
ROWSUM = [(9, 1, 29 * 1024 + 5), (8, 3, 32 * 1024), (1, 2, 256 * 1024 + 1), (2, 5, 1024), (2, 5, 1025)]
ROWSUM_REPEAT = 0


def partials_of(B, L):
    return B * ((L + SUM_CHUNK - 1) // SUM_CHUNK)


def rowsum_operand(B, C, L):
    """1 + N(0, 1) / 2: with a mean of 1 ONE lost sample of 262 145 already moves the sum by about four times the bound (the 257th partial of
    the long row holds a single sample); a zero-mean draw would leave that to the luck of the last sample's size"""
    return 1.0 + rnd(B, C, L, seed=seed_of(B, C, L), scale=0.5)


def rowsum_reference(g):
    return g.sum((0, 2)), RULE * g.abs().sum((0, 2))


# ---- TABLE UP: (B, Ci, Co, u, k, L, divide) ---------------------------------------------------------------------------------------------------------
UP = [(1, 16, 8, 2, 2, 33, 1.0), (2, 16, 8, 5, 11, 40, 3.0), (1, 32, 16, 3, 7, 257, 1.0), (1, 8, 4, 8, 16, 256, 3.0), (1, 8, 4, 4, 8, 1, 1.0)]
UP_REPEAT = 1


def up_operands(case):
    B, Ci, Co, u, k, L, div = case
    seed = seed_of(B, Ci, Co, u, k, L)
    return dict(w=rnd(Ci, Co, k, seed=seed) * (Ci * k / u) ** -0.5, g=rnd(B, Co, L * u, seed=seed + 1), x=rnd(B, Ci, L, seed=seed + 2))


def up_reference(case, g, x, w):
    """-> {'dx' (divided), 'dw' [Ci][Co][k], 'db'}: (want, bound)"""
    B, Ci, Co, u, k, L, div = case
    (wx, bx), dw, db = TH.conv_transpose_backward(g, x, w, u, SLOPE)
    return dict(dx=(wx / div, bx / div), dw=dw, db=db)


# ---- TABLE NOISE: (Lh, [(C, stride, K)]), B = 2 -----------------------------------------------------------------------------------------------------
NOISE = [(90, [(8, 6, 12)]), (90, [(8, 15, 30), (4, 3, 6), (2, 1, 1)]), (30, [(4, 15, 30)]), (31, [(4, 15, 30)]), (9, [(8, 6, 12)])]
NOISE_B = 2
NOISE_REPEAT = 1


def noise_geometry(Lh, s, K):
    pad = s // 2 if K > 1 else 0
    return pad, (Lh + 2 * pad - K) // s + 1


def noise_operands(Lh, stages):
    har = torch.tanh(rnd(NOISE_B, Lh, seed=seed_of(Lh, len(stages))))
    out = []
    for n, (C, s, K) in enumerate(stages):
        pad, Lo = noise_geometry(Lh, s, K)
        seed = seed_of(Lh, C, s, K, n)
        out.append(dict(C=C, s=s, K=K, pad=pad, Lo=Lo, w=rnd(C, K, seed=seed) * K ** -0.5, g=rnd(NOISE_B, C, Lo, seed=seed + 1)))
    return har, out


# ---- TABLE PWG ------------------------------------------------------------------------------------------------------------------------------------
PWG_AUX = (40, 64, 72, 128)
PWG_BLOCK = (2, 65, 4)                           # (B, L, dilation)
PWG_SPLITS = (16, 3, (3, 5))                     # (aux, B, L): 12 splits
PWG_REPEAT = (72, 0)


def pwg_cases():
    return [(aux, first) for aux in PWG_AUX for first in (1, 0)]


def pwg_block_weights(aux, seed):
    """tests/test_gpu_pwg_train.py's block_weights (imported: the one recipe)"""
    from tests.test_gpu_pwg_train import block_weights
    return block_weights(aux, seed)


def pwg_operands(aux, B, L):
    """one block's weights and the tensors of its forward, its data backward and its weight gradients; gate pre-activations drawn as
    tests/test_gpu_pwg_train.py draws them (1.5 N(0, 1))"""
    seed = seed_of(aux, B, L)
    c = dict(w=pwg_block_weights(aux, seed), x=rnd(B, 64, L, seed=seed + 1), c=rnd(B, aux, L, seed=seed + 2), prev=rnd(B, 64, L, seed=seed + 3),
             dxp=rnd(B, 64, L, seed=seed + 4), dS=rnd(B, 64, L, seed=seed + 5), a=rnd(B, 128, L, seed=seed + 6, scale=1.5),
             dc_prev=rnd(B, aux, L, seed=seed + 7), g=rnd(B, 64, L, seed=seed + 8), saved=rnd(B, 64, L, seed=seed + 9))
    return c


def pwg_forward_reference(w, x, c, dil):
    """the gate pre-activations a [B][128][L] of the block's first contraction -> (want, bound)"""
    a = F.conv1d(x, w['wc'].double(), w['bc'].double(), padding=dil, dilation=dil)
    ab = F.conv1d(x.abs(), w['wc'].double().abs(), w['bc'].double().abs(), padding=dil, dilation=dil)
    if c is not None:
        a, ab = a + F.conv1d(c, w['wa'].double()), ab + F.conv1d(c.abs(), w['wa'].double().abs())
    return a, RULE * ab


# ---- the whole module -----------------------------------------------------------------------------------------------------------------------------
V3 = dict(resblock='2', resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], upsample_initial_channel=128,
          upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8])
ODD = dict(upsample_rates=[5, 3, 2], upsample_kernel_sizes=[11, 7, 4], upsample_initial_channel=64)      # tests/test_gpu_voc_edges.py's ODD


def module_convolutions(h):
    """(channels, kernel, dilation, padding) of every resblock convolution of a configuration, stage by stage"""
    out = []
    for i in range(len(h['upsample_rates'])):
        ch = h['upsample_initial_channel'] // 2 ** (i + 1)
        for j, k in enumerate(h['resblock_kernel_sizes']):
            for d in TH.block_dils(h, j):
                out.append((ch, k, d, TH.get_padding(k, d)))
                if str(h['resblock']) == '1':
                    out.append((ch, k, 1, TH.get_padding(k, 1)))
    return out
