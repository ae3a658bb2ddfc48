"""Test infrastructure of the FastSpeech2 training objective (csrc/fs2_loss.hpp behind dsf_mel_loss / dsf_mel_loss_bwd / dsf_dur_loss /
dsf_dur_loss_bwd) at its tiles, seams and limits: the case tables of tests/test_gpu_fs2_loss_edges.py, seeded operands, the float64 (and fp32)
references and the yardstick.  Plain torch on the CPU.  tests/test_fs2_loss_edges_host.py asserts that the tables hold what they claim, runs
every reference once and shows that the yardstick catches the faults the shapes exist for.

Nothing is re-derived: the references are tests/fs2_loss_helpers.py's ssim_map, l1_loss, ssim_loss and dur_loss.  Added here is only what the
C ABI exposes and they lack - the unweighted means, the map as an output, sum(map * R) for grad_map and the combination of grad_out[0..2] with
a grad_map.  kMlTile, kMlMaxM, kDurMaxTxt and the 256-thread block width are parsed from the header's text.

THE YARDSTICK (tests/test_gpu_fs2_loss.py's rule and floors): the device's distance from float64 is held to
max(2 x the CPU fp32 restatement's own distance from float64, floor), floors 1e-5 on the mel values and the map, 2e-7 on the mel gradient,
1e-6 on the duration values and gradient.  For the map and the gradients the rule is applied PER ROW (a frame of the mel tensors, an utterance
of the duration gradient): both distances are the row's largest error, the floor is relative to that row's largest float64 magnitude, so that
a seam frame of small magnitude cannot hide behind the bulk.  A row whose float64 reference is all zero and whose restatement is exact owes
exact zeros.  ratio = distance / allowance; a case passes at <= 1."""
import functools
import os
import re
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import fs2_loss_helpers as LH

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffsinger_amd', 'csrc', 'fs2_loss.hpp')
GUARD = 64                                       # NaN floats either side of every buffer
WINDOW = 11                                      # fs2_loss_helpers.ssim_map's window: halo 5 forward, 10 backward
HALO = WINDOW // 2
FLOOR_MEL_VALUE, FLOOR_MEL_GRAD, FLOOR_DUR = 1e-5, 2e-7, 1e-6
SIL = (1, 2, 7)


def header_constant(name):
    """`constexpr int <name> = <integer>;` parsed from csrc/fs2_loss.hpp"""
    with open(HEADER) as f:
        m = re.search(r'constexpr\s+int\s+' + re.escape(name) + r'\s*=\s*([0-9]+)\s*;', f.read())
    assert m, f'{name} is not a constant of fs2_loss.hpp'
    return int(m.group(1))


def launch_bounds(kernel):
    """the N of `__launch_bounds__(N) void <kernel>(` in csrc/fs2_loss.hpp"""
    with open(HEADER) as f:
        m = re.search(r'__launch_bounds__\((\d+)\)\s+void\s+' + re.escape(kernel) + r'\s*\(', f.read())
    assert m, f'{kernel} has no launch bounds in fs2_loss.hpp'
    return int(m.group(1))


TILE, MAX_M, MAX_TXT = header_constant('kMlTile'), header_constant('kMlMaxM'), header_constant('kDurMaxTxt')
BLOCK = launch_bounds('k_dur_loss_rows')         # phones are scanned in 256 chunks of ceil(T_txt / 256)
FINAL_BLOCK = launch_bounds('k_mel_loss_final')  # the partials are summed by 256 threads, strided


def gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def tiles(T):
    return (T + TILE - 1) // TILE


def chunk_of(Tt):
    return (Tt + BLOCK - 1) // BLOCK


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
def row_ratio(got, ref64, ref32, floor):
    """-> (worst ratio, its row, that row's device distance, that row's allowance): the rule per row of the last axis.
    allowance[r] = max(2 e32[r], floor scale[r]): e32[r] the restatement's largest error in the row, scale[r] the row's largest float64
    magnitude"""
    M = ref64.shape[-1]
    g, r64, r32 = (t.detach().double().cpu().reshape(-1, M) for t in (got, ref64, ref32))
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    e_dev, e_32, scale = (g - r64).abs().amax(-1), (r32 - r64).abs().amax(-1), r64.abs().amax(-1)
    e_dev = torch.where(torch.isfinite(e_dev), e_dev, torch.full_like(e_dev, float('inf')))
    allow = torch.maximum(2 * e_32, floor * scale)
    r = torch.where(allow > 0, e_dev / allow.clamp(min=1e-300), torch.where(e_dev == 0, torch.zeros_like(e_dev), torch.full_like(e_dev, float('inf'))))
    i = int(r.argmax())
    return float(r[i]), i, float(e_dev[i]), float(allow[i])


def value_ratio(got, ref64, ref32, floor, least=0.0):
    """the rule on one number: |got - ref64| / max(2 |ref32 - ref64|, floor max(|ref64|, least))"""
    got, ref64, ref32 = float(got), float(ref64), float(ref32)
    e_dev = abs(got - ref64) if got == got else float('inf')
    allow = max(2 * abs(ref32 - ref64), floor * max(abs(ref64), least))
    return (e_dev / allow if allow > 0 else (0.0 if e_dev == 0 else float('inf'))), e_dev, allow


# ---- TABLE MEL: (B, T, M, bias, zero-frame pattern, stride layout) ----------------------------------------------------------------------
MelCase = namedtuple('MelCase', 'B T M bias zero layout')
LAYOUTS = ('contig', 'cwt', 'rows', 'mixed')     # cwt: [:, :, :M] of [B, T, M + 1]; rows: [:, 2:T + 2] of [B, T + 3, M]; mixed: x cwt, y rows
MEL_T = (1, 5, 6, 10, 11, 15, 16, 17, 21, 26, 27, 31, 32, 33, 48)
MEL_M = (1, 5, 10, 11, 12, 127, 128)
MEL_PARTIALS = (4080, 4096, 4097)                # / 16: 255, 256, 257 partials of k_mel_loss_final's strided loop
ZERO_PATTERNS = ('z0', 'z15', 'z16', 'z15_16', 'zlast', 'run10_21', 'run6_27', 'lastbin', 'negzero', 'utt')
ZERO_T = (33, 48)


def mel_cases():
    out = []
    for i, T in enumerate(MEL_T):                                               # 'tail': fs2_loss_helpers.mel_case's padding frames
        out.append(MelCase((3, 1)[i % 2], T, 80, 6.0, 'tail', LAYOUTS[i % 4]))
    for i, M in enumerate(MEL_M):
        out.append(MelCase((3, 1)[i % 2], 33, M, 6.0, 'tail', LAYOUTS[(i + 1) % 4]))
    out.append(MelCase(3, 33, 10, 20.0, 'tail', 'cwt'))                         # the live cwt_loss: ssim view
    out += [MelCase(1, T, 8, 6.0, 'tail', 'contig') for T in MEL_PARTIALS]
    n = 0
    for T in ZERO_T:
        for z in ZERO_PATTERNS:
            out.append(MelCase(3 if z == 'utt' else (1, 3)[n % 2], T, 80, 6.0, z, LAYOUTS[n % 4]))
            n += 1
    out += [MelCase(3, 33, 80, 6.0, 'tail', lay) for lay in ('contig', 'cwt', 'mixed_rev')]       # every layout at one shape (rows, mixed: above)
    return out


def mel_id(c):
    return f'B{c.B}-T{c.T}-M{c.M}-bias{c.bias:g}-{c.zero}-{c.layout}'


def zero_frames(pattern, T):
    """the target frames a pattern empties"""
    return {'tail': [], 'z0': [0], 'z15': [15], 'z16': [16], 'z15_16': [15, 16], 'zlast': [T - 1], 'run10_21': list(range(10, 22)),
            'run6_27': list(range(6, 28)), 'lastbin': [15, 16, 17], 'negzero': [0, 16], 'utt': []}[pattern]


def mel_operands(c):
    """mel_out x / target y [B, T, M] fp32, seeded.  A pattern's frames are emptied in every utterance of the target; mel_out keeps its
    prediction there (the weights must drop it) except in utterance 0 of a batch of three."""
    x, y = LH.mel_case(c.B, c.T, c.M, seed=c.B * 100000 + c.T * 131 + c.M, bias_scale=1.0 if c.bias == 6.0 else 0.5)
    fr = [t for t in zero_frames(c.zero, c.T) if t < c.T]
    if fr:
        y[:, fr] = 0.0
        if c.B > 1:
            x[0, fr] = 0.0
    if c.zero == 'lastbin':
        y[:, 16, c.M - 1] = -3.7                                                # the frame's only nonzero bin is the last one: it counts
    if c.zero == 'negzero':
        y[:, fr] = -0.0                                                         # -0.0 != 0 is false: the frame does not count
    if c.zero == 'utt':
        y[c.B - 1] = 0.0                                                        # one utterance entirely zero (its prediction is not) beside normal ones
    assert float(LH.weights_nonzero_speech(y).sum()) > 0, 'a batch without a weighted frame: the reference is 0 / 0'
    # (the all-zero-target BATCH is not in the table: the kernel returns 0 / 0 = NaN values like torch, but a zero gradient where torch has NaN)
    return x, y


def mel_weights(y):
    return LH.weights_nonzero_speech(y)


def mel_reference(x, y, bias, terms=3, weighted=1, lam=(1.0, 1.0), gout=(1.0, 1.0, 0.0), R=None, dtype=torch.float64):
    """dsf_mel_loss / dsf_mel_loss_bwd restated on fs2_loss_helpers: -> dict(out [4], map [B,T,M] or None, dx [B,T,M]).
    out = [lam_l1 L1, lam_ssim (1 - S), mean S, count]; dx = d/dx of gout . out[0..2] + sum(map * R)."""
    xr, yy = x.detach().to(dtype).clone().requires_grad_(True), y.detach().to(dtype)
    zero = xr.sum() * 0
    w = mel_weights(yy) if weighted else torch.ones_like(yy)
    smap, o0, o1, o2 = None, zero, zero, zero
    if terms & 1:
        o0 = (LH.l1_loss(xr, yy) if weighted else F.l1_loss(xr, yy)) * lam[0]
    if terms & 2:
        smap = LH.ssim_map(xr[:, None] + bias, yy[:, None] + bias).mean(1)
        if weighted:
            o1 = LH.ssim_loss(xr, yy, bias) * lam[1]
            o2 = (smap * w).sum() / w.sum()
        else:
            o1, o2 = (1 - smap).mean() * lam[1], smap.mean()                    # the ssim() drop-in: the unweighted mean of S
    total = gout[0] * o0 + gout[1] * o1 + gout[2] * o2
    if R is not None:
        total = total + (smap * R.to(dtype)).sum()
    total.backward()
    out = torch.stack([o0.detach(), o1.detach(), o2.detach(), w.sum()])
    return dict(out=out, map=None if smap is None else smap.detach(), dx=xr.grad)


@functools.lru_cache(maxsize=None)
def mel_case_reference(c, dtype):
    """every table row's reference, computed once: terms 3, weighted, grad_out (1, 1, 0.25), a seeded grad_map"""
    x, y = mel_operands(c)
    return mel_reference(x, y, c.bias, 3, 1, MEL_LAM, MEL_GOUT, mel_grad_map(c), dtype)


MEL_LAM, MEL_GOUT = (0.5, 0.5), (1.0, 1.0, 0.25)      # (0.25 - 0.5 * 1) / count on S: the two SSIM outputs do not cancel


def mel_grad_map(c):
    """dL/dS of a table row: small beside the loss's own 1 / count, and present on unweighted frames too"""
    return torch.randn(c.B, c.T, c.M, generator=gen(c.B, c.T, c.M, 7)) / (c.B * c.T * c.M)


# ---- TABLE DUR: (B, T_txt, T, segmentation, pattern) ------------------------------------------------------------------------------------
DurCase = namedtuple('DurCase', 'B Tt T seg pat')
DUR_TT = (1, 2, 255, 256, 257, 511, 512, 513, 2047, 2048)
DUR_T_AT_12 = (1, 255, 256, 257)
SEGS = ('sil', 'wdb')
NAN_PATTERNS = ('wdb_overflow',)


def dur_cases():
    out, n = [], 0
    for Tt in DUR_TT:                                                           # a word straddles every chunk seam where a chunk holds >= 2 phones
        for seg in SEGS:
            out.append(DurCase((1, 3)[n % 2], Tt, max(3, 3 * Tt), seg, 'straddle' if chunk_of(Tt) > 1 else 'random'))
            n += 1
    for T in DUR_T_AT_12:
        for seg in SEGS:
            out.append(DurCase((3, 1)[n % 2], 12, T, seg, 'random'))
            n += 1
    for Tt in (12, 513):
        for seg in SEGS:
            out.append(DurCase((1, 3)[n % 2], Tt, 3 * Tt, seg, 'one_word'))
            out.append(DurCase(3, Tt, 3 * Tt, seg, 'pad_row'))
            out.append(DurCase(3, Tt, 3 * Tt, seg, 'dur_edge'))
            n += 1
        out += [DurCase(3, Tt, 3 * Tt, 'sil', 'sil_edges'), DurCase(3, Tt, 3 * Tt, 'sil', 'row_nosil'),
                DurCase(1, Tt, 3 * Tt, 'wdb', 'all_ones'), DurCase(3, Tt, 3 * Tt, 'wdb', 'wdb_two'), DurCase(3, Tt, 3 * Tt, 'wdb', 'wdb_overflow')]
    out += [DurCase(3, MAX_TXT, 3 * MAX_TXT, 'wdb', 'all_ones'), DurCase(1, MAX_TXT, 3 * MAX_TXT, 'wdb', 'wdb_overflow')]
    for seg in SEGS:
        out += [DurCase(3, 12, 40, seg, 'zero_frames'), DurCase(3, 12, 3040, seg, 'long_phone'), DurCase(1, 12, 3040, seg, 'long_phone')]
    return out


def dur_id(c):
    return f'B{c.B}-Tt{c.Tt}-T{c.T}-{c.seg}-{c.pat}'


def dur_flags(c):
    """nan: the header's `bad` path (all losses and gradients NaN).  no_word: one phone under silence ids has no kept word - wdur is 0 / 0 in
    torch and on the device alike, and only pdur, sdur and their gradient are compared."""
    return dict(nan=c.pat in NAN_PATTERNS, no_word=c.seg == 'sil' and c.Tt == 1)


def dur_operands(c):
    """-> dict(dur_pred [B,Tt] fp32, mel2ph [B,T], tok [B,Tt], wdb [B,Tt] or None, sil list or None), seeded"""
    B, Tt, T, seg, pat = c
    g = gen(B, Tt, T, SEGS.index(seg), sum(map(ord, pat)))
    chunk, mid = chunk_of(Tt), Tt // 2
    tok = torch.randint(8, 40, (B, Tt), generator=g)
    nvalid = [Tt] * B
    if Tt >= 5 and pat in ('random', 'straddle', 'pad_row', 'zero_frames', 'wdb_two', 'dur_edge'):
        for b in range(1, B):                                                   # padded phones at the end of the later rows
            nvalid[b] = Tt - b * Tt // 5
            tok[b, nvalid[b]:] = 0
    valid = tok > 0
    seams = [k for k in range(chunk, Tt, chunk)] if chunk > 1 else []
    wdb = None
    if seg == 'sil':
        silm = torch.rand(B, Tt, generator=g) < 0.15
        if pat == 'one_word':
            silm[:] = False
        if pat == 'straddle':
            for k in seams:
                silm[:, k - 1:k + 1] = False                                    # a non-silence run across every seam
        silm[:, 0] = Tt > 1                                                     # word 0 is dropped: a silence first, so that words are kept
        if Tt > 1:
            silm[:, mid] = False                                                # the phone that is given a frame below
        if pat == 'dur_edge':
            silm[:, 1:4] = False
        if pat == 'sil_edges':
            silm[:, [Tt - 1, Tt // 3, Tt // 3 + 1]] = True                      # first (above), last, two adjacent
        if pat == 'row_nosil':
            silm[1] = False                                                     # a row with no silence: no kept word in it
        silm &= valid
        tok[silm] = torch.tensor(SIL)[torch.randint(0, len(SIL), (int(silm.sum()),), generator=g)]
    else:
        wdb = (torch.rand(B, Tt, generator=g) < 0.4).long()
        if pat == 'one_word':
            wdb[:] = 0
        if pat in ('all_ones', 'wdb_overflow'):
            wdb[:] = 1                                                          # every phone its own word: the last one in slot T_txt - 1
        if pat == 'straddle':
            for k in seams:
                wdb[:, k - 1] = 0                                               # phones k - 1 and k in one word
        wdb *= valid.long()
        wdb[:, -1] = 0
        if pat == 'wdb_two':
            wdb[:, Tt // 3] = 2                                                 # skips a slot; the running count stays below T_txt
        if pat == 'wdb_overflow':
            wdb[B - 1, 1] = 2                                                   # the last phone's running count reaches T_txt
    mel2ph = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        n = T if b == 0 else max(1, T - b * (T // 4))
        if pat == 'long_phone' and b == 0:
            ph = torch.cat([torch.full((3000,), 5), torch.randint(1, nvalid[b] + 1, (n - 3000,), generator=g)])
        else:
            ph = torch.randint(1, nvalid[b] + 1, (n,), generator=g)
        ph[n - 1] = min(mid + 1, nvalid[b])                                     # a frame on a phone of a kept word
        if pat == 'zero_frames':
            ph[ph == 3] = 4                                                     # phones 3 and 7 (1-based) hold no frame
            ph[ph == 7] = 8
        mel2ph[b, :n] = ph.sort().values
    if pat == 'pad_row':
        mel2ph[1] = 0                                                           # a row of all-padding mel2ph beside normal rows
    dur_gt = LH.mel2ph_to_dur(mel2ph, Tt).float() * valid.float()
    dur_pred = ((dur_gt + 1).log() + 0.3 * torch.randn(B, Tt, generator=g)).float()
    if pat == 'dur_edge':
        dur_pred[:, 1], dur_pred[:, 2], dur_pred[:, 3] = 0.0, -0.5, -3.0        # clamp(min=0)'s edge and both sides of it
        dur_pred[0, 0] = 0.0
    return dict(dur_pred=dur_pred, mel2ph=mel2ph, tok=tok, wdb=wdb, sil=list(SIL) if seg == 'sil' else None)


DUR_LAM = dict(lam_ph=0.7, lam_word=1.3, lam_sent=0.9)


def dur_gout(c):
    return [float(v) for v in (0.5 + torch.rand(3, generator=gen(c.B, c.Tt, c.T, 3)))]


def word_slots(o):
    """[B, Tt] slot of every phone's word (-1: in no kept word), as fs2_loss_helpers.dur_loss indexes its scatter_add"""
    tok = o['tok']
    if o['wdb'] is not None:
        return F.pad(o['wdb'].cumsum(1), (1, 0))[:, :-1]
    is_sil = torch.zeros_like(tok).bool()
    for p in o['sil']:
        is_sil |= tok == p
    return (is_sil.long().cumsum(-1) * (~is_sil).long()) - 1


def dur_counts(o):
    """(phones, kept words with frames) of a case"""
    Tt = o['tok'].shape[1]
    dur_gt = LH.mel2ph_to_dur(o['mel2ph'], Tt) * (o['tok'] > 0)
    s = word_slots(o)
    per = torch.zeros(s.shape[0], Tt + 1, dtype=torch.long).scatter_add(1, (s + 1).clamp(max=Tt), dur_gt)[:, 1:]
    return int((o['tok'] > 0).sum()), int((per > 0).sum())


def dur_reference(o, gout, dtype=torch.float64, drop_wdur=False, lam=None):
    """-> dict(out [3], grad [B,Tt]): fs2_loss_helpers.dur_loss and the gradient of gout . out"""
    lam = lam or DUR_LAM
    dr = o['dur_pred'].to(dtype).clone().requires_grad_(True)
    kw = dict(wdb=o['wdb']) if o['wdb'] is not None else dict(sil_ids=o['sil'])
    L = LH.dur_loss(dr, o['mel2ph'], o['tok'], **kw, **lam)
    keys = [k for k in ('pdur', 'wdur', 'sdur') if not (drop_wdur and k == 'wdur')]
    sum(gout[('pdur', 'wdur', 'sdur').index(k)] * L[k] for k in keys).backward()
    return dict(out=torch.stack([L[k].detach() for k in ('pdur', 'wdur', 'sdur')]), grad=dr.grad)


@functools.lru_cache(maxsize=None)
def dur_case_reference(c, dtype):
    f = dur_flags(c)
    assert not f['nan']
    return dur_reference(dur_operands(c), dur_gout(c), dtype, drop_wdur=f['no_word'])
