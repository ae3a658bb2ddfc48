"""Edge cases of the STFT family (include/dsv.h section "STFT", csrc/voc_stft.hpp, csrc/voc_stft_abi.hpp): the case lists that
tests/test_gpu_stft_edges.py runs on the device and tests/test_stft_edges_host.py replays on the CPU, the float64 restatements the cases are
judged by, the bounds, and float32 restatements of the kernels' INDEX ARITHMETIC with switches for restated bugs ("mutants").  CPU only, built
from torch and numpy - never from diffsinger_amd.stft.

    ref_istft_ola64        the inverse as the header text of include/dsv.h states it (accepts what torch.istft refuses)
    inverse_yardstick32    the windowed frames of the inverse as a float32 torch.matmul against a basis built in float64 and rounded HERE
    soft_threshold64       S * max(|S| - v, 0) / |S|
    single_reflection64    the padded signal of a ragged row as the `lengths` paragraph of include/dsv.h states it
    restate_stft32 / restate_logmel32 / restate_ola32
                           the staging (rows of RL samples, chunks of KC), the mel product and the gather, in float32, with the mutants:
        'a' the last frame of a 64-frame workgroup is read one LDS row (one hop) further
        'b' the row wrap of the B read advances one sample short when RL is odd
        'c' the Nyquist weight is left out of the mel
        'd' a ragged row reflects about L instead of its own end
        'e' the overlap-add loses its last contributing frame (fhi one short)
        'f' the window sum runs over all frames instead of the row's frame_counts
        'g' the second and later KC chunks are staged from n0 = 0

Bounds (none measured on the device):
    spectra, magnitudes, log-mels   2 x the error of SH.yardstick32 on the case's own input against the same float64 reference
    windowed frames of the inverse  2 x the error Y of inverse_yardstick32
    inverse output, per sample t    (n_f(t) 2 Y + 8 u sum_f |frame64|) / wss64(t) + 8 u |out64(t)|,  u = 2^-24;  exactly 0 where wss64(t) = 0
                                    and beyond the row's signal.  The 8s are a condition: fewer than 8 float32 additions in the gather and
                                    in the window sum, one division
    spectral subtraction            |S' - soft64(S64)| <= 2 x forward yardstick + 4 u |S64| element-wise (soft thresholding is the proximal map
                                    of v |.|, hence nonexpansive); exactly 0 where |S64| < v - 2 x yardstick"""
import functools
from unittest import mock

import numpy as np
import torch

from tests import stft_helpers as SH

U = 2.0 ** -24
NF_WG = 64                        # frames per workgroup (kStftNF)
LDS_BUDGET = 72 * 1024            # kStftLdsBudget
ROWS = 4                          # every forward case compares at least this many rows: the yardstick's maximum is a fair sample



def cerr(got, want):
    """max-abs over re and im"""
    d = torch.view_as_real(torch.as_tensor(got).to(torch.complex128).cpu()) - torch.view_as_real(torch.as_tensor(want).to(torch.complex128))
    return float(d.abs().max())


def plan(n_fft, hop):
    """stft_plan of csrc/voc_stft_abi.hpp: (KC, RL) - the largest power-of-two chunk whose 64-frame window fits the LDS budget"""
    KC = n_fft
    while KC >= 8:
        RL = min(hop, KC)
        if (NF_WG - 1 + (KC + RL - 1) // RL) * (RL + 2) * 4 <= LDS_BUDGET:
            return KC, RL
        KC >>= 1
    return 8, min(hop, 8)


def row_groups(n_fft, GT=2):
    """ngroups of k_stft<MODE, GT>: a wave holds GT row tiles of 32 rows, four waves a group"""
    return (n_fft // 32 + 4 * GT - 1) // (4 * GT)


def zsplit(n_frames, B, n_fft, GT=2):
    """stft_zsplit of csrc/voc_stft_abi.hpp: grid.z of dsv_stft / dsv_istft (GT = 2) - the row groups are split over grid.z until the launch has
    512 workgroups, at most one group per z.  With z < ngroups a workgroup LOOPS over row groups: it reuses the staged window when the
    contraction is one chunk and re-stages every chunk behind a barrier when it is not."""
    have = (n_frames + NF_WG - 1) // NF_WG * B
    z = 1 if have >= 512 else (512 + have - 1) // have
    return min(z, row_groups(n_fft, GT))


# (n_fft, hop, win, B, frames per row): launches of >= 512 workgroups, which stft_zsplit leaves unsplit.  256/64/256 has ONE row group: no launch of
# it is ever split and its workgroups never loop; 512/128/512 has two groups (one chunk: the staged window is reused across them), 2048/300/1200
# eight (chunks of KC = 256: every chunk is staged again for every group).  A B = 1 call of the latter two is split over grid.z.
UNSPLIT_CASES = [(256, 64, 256, 64, 512), (512, 128, 512, 64, 512), (2048, 300, 1200, 512, 8)]
UNSPLIT_INVERSE = (512, 128, 512, 64, 512)        # the inverse at 512: two row groups, two chunks of 256 spectrum slots


def row_frames(length, n_fft, hop, pl, pr):
    """the header formula: 1 + (len + pad_l + pad_r - n_fft) / hop, 0 when that is not one frame"""
    tot = length + pl + pr
    return 0 if length < 1 or tot < n_fft else 1 + (tot - n_fft) // hop


# ------------------------------------------------------------------------------------------------------------------------------------
# forward cases
# ------------------------------------------------------------------------------------------------------------------------------------
FORWARD_GEOMS = [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200), (2048, 300, 1200), (256, 256, 256), (256, 75, 255), (256, 1, 256),
                 (1024, 256, 200)]
FRAME_COUNTS = (1, 63, 64, 65, 129)
OLD_GEOMS = [(512, 128, 512), (1024, 256, 1024), (1024, 256, 800), (2048, 512, 2048), (256, 64, 256)]        # tests/test_gpu_stft.py SHAPES


def forward_cases(n_fft, hop, win):
    """[(frames, L, center, pad_mode)]: every frame count hit exactly and one sample short of the next frame (center=False), one centred
    constant and one centred reflect case"""
    out = []
    for T in FRAME_COUNTS:
        L = n_fft + hop * (T - 1)
        out.append((T, L, False, 'constant'))
        if hop > 1:
            out.append((T, L + hop - 1, False, 'constant'))
    Lc = max(65 * hop + 3, n_fft // 2 + 5)
    out += [(1 + Lc // hop, Lc, True, 'constant'), (1 + Lc // hop, Lc, True, 'reflect')]
    return out


def old_forward_cases(n_fft, hop, win):
    """the L = 9000 cases of tests/test_gpu_stft.py::test_forward_against_float64 (for the question which mutants the old shapes see)"""
    return [(None, 9000, c, m) for m in ('constant', 'reflect') for c in (True, False)]


def forward_case(n_fft, hop, win, T, L, center, mode, rows=ROWS):
    wav = SH.make_signal(L, seed=L + n_fft + hop, batch=rows)
    want = SH.ref_stft64(wav, n_fft, hop, win, center, mode)
    assert T is None or want.shape[2] == T, (want.shape, T)
    yard = cerr(SH.yardstick32(wav, n_fft, hop, win, center, mode), want)
    return dict(wav=wav, want=want, yard=yard)


# ------------------------------------------------------------------------------------------------------------------------------------
# float32 restatement of the forward staging
# ------------------------------------------------------------------------------------------------------------------------------------
def _sample_index(pos, length, L, pl, pr, reflect, mutant):
    """stft_sample: padded positions (int64 array) -> (index into the row's buffer, valid)"""
    u = pos - pl
    ok = u < length + pr
    outside = (u < 0) | (u >= length)
    if reflect:
        end = L if mutant == 'd' else length
        v = np.where(u < 0, -u, 2 * (end - 1) - u)
        ok = ok & np.where(outside, (v >= 0) & (v < end), True)
        u = np.where(outside, v, u)
    else:
        ok = ok & ~outside
    return np.where(ok, u, 0), ok


@functools.lru_cache(maxsize=4)
def _dft_basis32(n_fft, win):
    return SH.dft_basis32(n_fft, win).reshape(n_fft, -1)


def restate_stft32(wav, n_fft, hop, win, center=True, pad_mode='constant', pad=None, lengths=None, clamp=False, mutant=None):
    """complex64 [B][n_bins][T]: the kernel's staging restated.  A workgroup owns frames f0 .. f0 + 63; per chunk [n0, n0 + KC) it stages LDS
    rows of RL samples, row i starting at padded position (f0 + i) hop + n0, and frame f0 + j reads sample n0 + m from row j + m / RL, column
    m mod RL.  The contraction is a float32 matmul per chunk with float64 totals across chunks; frames at or beyond a row's count are 0."""
    x = torch.as_tensor(wav).to(torch.float32)
    if x.dim() == 1:
        x = x[None]
    if clamp:
        x = x.clamp(-1.0, 1.0)
    x = x.numpy()
    B, L = x.shape
    pl, pr = SH._pads(n_fft, center, pad)
    reflect = pad_mode == 'reflect'
    KC, RL = plan(n_fft, hop)
    T = 1 + (L + pl + pr - n_fft) // hop
    f = np.arange(T, dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    f0 = f // NF_WG * NF_WG
    j = f - f0
    n0 = n // KC * KC
    m = n - n0
    row, col = j + m // RL, m % RL
    if mutant == 'a':
        row = row + (j == NF_WG - 1)
    if mutant == 'b' and RL % 2:
        col = col - m // RL
    if mutant == 'g':
        n0 = 0 * n0
    pos = (f0 + row) * hop + n0 + col
    frames = np.zeros((B, T, n_fft), np.float32)
    counts = []
    for b in range(B):
        length = L if lengths is None else min(max(int(lengths[b]), 0), L)
        idx, ok = _sample_index(pos, length, L, pl, pr, reflect, mutant)
        frames[b] = np.where(ok, x[b][idx], np.float32(0))
        counts.append(min(row_frames(length, n_fft, hop, pl, pr), T))
    D = _dft_basis32(n_fft, win)
    fr = torch.from_numpy(frames)
    acc = torch.zeros(B, T, D.shape[1], dtype=torch.float64)
    for c0 in range(0, n_fft, KC):
        acc += torch.matmul(fr[:, :, c0:c0 + KC], D[c0:c0 + KC]).double()
    Y = acc.to(torch.float32).reshape(B, T, 2, -1)
    for b, t in enumerate(counts):
        Y[b, t:] = 0
    return torch.complex(Y[:, :, 0], Y[:, :, 1]).transpose(1, 2), counts


def flavour_options(flavour, over, n_fft, hop, eps=1e-10):
    """the options of a flavour of tests/stft_helpers.py with the operator's overrides (logmel_op(..., **over)) applied - a local copy"""
    return dict(SH._flavour(flavour, n_fft, hop, eps), **(over or {}))


def restate_logmel32(wav, basis, flavour, n_fft, hop, win, eps=1e-10, mutant=None, over=None):
    """(log-mel, magnitude) float32 [B][T][.] from restate_stft32: mel = mag . basis^T with the Nyquist column as one more step"""
    o = flavour_options(flavour, over, n_fft, hop, eps)
    S, _ = restate_stft32(wav, n_fft, hop, win, o['center'], o['pad_mode'], o['pad'], clamp=o['clamp'], mutant=mutant)
    S = S.transpose(1, 2)
    mag = torch.sqrt(S.real * S.real + S.imag * S.imag + np.float32(o['mag_eps']))
    bt = torch.as_tensor(basis).to(torch.float32).clone()
    if mutant == 'c':
        bt[:, n_fft // 2] = 0
    mel = torch.matmul(mag, bt.t())
    clipped = torch.clamp(mel, min=float(np.float32(o['floor']))).double()                 # the log in float64, rounded once
    return (torch.log10(clipped) if o['log10'] else torch.log(clipped)).to(torch.float32), mag


# ------------------------------------------------------------------------------------------------------------------------------------
# inverse
# ------------------------------------------------------------------------------------------------------------------------------------
INVERSE_GEOMS = [(512, 128, 512), (1024, 256, 800), (2048, 240, 1200), (256, 256, 256), (256, 75, 255), (1024, 256, 200)]
INVERSE_FRAMES = (1, 2, 65)


def ref_istft_ola64(S, n_fft, hop, win, center=True, length=None, frame_counts=None):
    """include/dsv.h, dsv_istft: irfft of every frame (imaginary parts of bins 0 and n_fft / 2 ignored) x window, overlap-added, divided by the
    window sum of squares ONLY where that is positive, n_fft / 2 trimmed per side when center, zeros beyond the row's signal.
    S complex [B][n_bins][nF].  Returns (out [B][length], windowed frames [B][nF][n_fft] (0 at and beyond a row's frame count), and per
    output sample: window sum of squares, sum of |contributing frame values|, number of contributing frames (window > 0)) - all float64."""
    S = torch.as_tensor(S).to(torch.complex128).numpy()
    if S.ndim == 2:
        S = S[None]
    B, n_bins, nF = S.shape
    assert n_bins == n_fft // 2 + 1
    X = S.transpose(0, 2, 1).copy()
    X[..., 0] = X[..., 0].real
    X[..., -1] = X[..., -1].real
    w = SH.window64(n_fft, win).numpy()
    frames = np.fft.irfft(X, n=n_fft, axis=-1) * w
    fc = [nF] * B if frame_counts is None else [min(max(int(c), 0), nF) for c in frame_counts]
    trim = n_fft // 2 if center else 0
    total = n_fft + hop * (nF - 1)
    if length is None:
        length = max(total - 2 * trim, 0)
    out, wss, ab, cnt = (np.zeros((B, length)) for _ in range(4))
    for b in range(B):
        frames[b, fc[b]:] = 0.0
        buf, ws, a, c = (np.zeros(total) for _ in range(4))
        for f in range(fc[b]):
            s = slice(f * hop, f * hop + n_fft)
            buf[s] += frames[b, f]
            ws[s] += w * w
            a[s] += np.abs(frames[b, f])
            c[s] += w > 0
        n = 0 if fc[b] == 0 else max(min(length, n_fft + hop * (fc[b] - 1) - 2 * trim), 0)
        s = slice(trim, trim + n)
        pos = ws[s] > 0
        out[b, :n] = np.where(pos, buf[s] / np.where(pos, ws[s], 1.0), buf[s])
        wss[b, :n], ab[b, :n], cnt[b, :n] = ws[s], a[s], c[s]
    return out, frames, wss, ab, cnt


@functools.lru_cache(maxsize=4)
def inverse_basis64(n_fft, win):
    """[n_fft][n_fft] float64, row n; columns (Re 0 .. Re n_fft/2 | Im 1 .. Im n_fft/2 - 1): window / n_fft, the factor 2 of the interior bins"""
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % n_fft).astype(np.float64) / n_fft
    w = SH.window64(n_fft, win).numpy()[:, None] / n_fft
    ck = np.full(n_fft // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    return np.concatenate([w * ck * np.cos(ang), (-2.0 * w * np.sin(ang))[:, 1:-1]], axis=1)


def spectrum_rows(S):
    """complex [B][n_bins][nF] -> real [B][nF][n_fft] in the column order of inverse_basis64 (Im of bins 0 and n_fft / 2 dropped)"""
    S = torch.as_tensor(S)
    return torch.cat([S.real, S.imag[:, 1:-1]], dim=1).transpose(1, 2)


@functools.lru_cache(maxsize=4)
def _inverse_basis32(n_fft, win):
    return torch.from_numpy(inverse_basis64(n_fft, win).astype(np.float32))


def inverse_yardstick32(S, n_fft, win, frame_counts=None):
    """windowed frames [B][nF][n_fft] as a float32 torch.matmul on the CPU"""
    S = torch.as_tensor(S).to(torch.complex64)
    Binv = _inverse_basis32(n_fft, win)
    fr = torch.matmul(spectrum_rows(S).contiguous(), Binv.t())
    if frame_counts is not None:
        for b, c in enumerate(frame_counts):
            fr[b, min(max(int(c), 0), fr.shape[1]):] = 0
    return fr


def inverse_bound(out64, wss, ab, cnt, Y):
    """per-sample bound of the inverse output; 0 (exact) where the window sum is 0 and beyond the row's signal"""
    pos = wss > 0
    return np.where(pos, (cnt * 2.0 * Y + 8.0 * U * ab) / np.where(pos, wss, 1.0) + 8.0 * U * np.abs(out64), 0.0)


def restate_ola32(frames32, n_fft, hop, win, center, length, frame_counts=None, mutant=None):
    """k_istft_ola: every output sample adds its contributing frames flo .. fhi in ascending order in float32, forms the window sum the same
    way and divides where that exceeds FLT_MIN"""
    fr = np.asarray(frames32, dtype=np.float32)
    B, nF, _ = fr.shape
    wsq = (SH.window64(n_fft, win).numpy() ** 2).astype(np.float32)
    trim = n_fft // 2 if center else 0
    out = np.zeros((B, length), np.float32)
    t = np.arange(length, dtype=np.int64) + trim
    for b in range(B):
        nfb = nF if frame_counts is None else min(max(int(frame_counts[b]), 0), nF)
        if nfb == 0:
            continue
        live = t < n_fft + hop * (nfb - 1) - trim
        flo = np.where(t - n_fft + 1 <= 0, 0, (t - n_fft + hop) // hop)
        fhi = np.minimum(t // hop, nfb - 1) - (1 if mutant == 'e' else 0)
        whi = np.minimum(t // hop, nF - 1) if mutant == 'f' else fhi
        s, ws = np.zeros(length, np.float32), np.zeros(length, np.float32)
        for f in range(nF):
            nn = np.clip(t - f * hop, 0, n_fft - 1)
            s = np.where(live & (f >= flo) & (f <= fhi), s + fr[b, f][nn], s).astype(np.float32)
            ws = np.where(live & (f >= flo) & (f <= whi), ws + wsq[nn], ws).astype(np.float32)
        big = ws > np.finfo(np.float32).tiny
        out[b] = np.where(big, s / np.where(big, ws, np.float32(1)), s)
    return out


def inverse_case(n_fft, hop, win, T, rows=ROWS):
    """complex64 spectra [rows][n_bins][T] of a real signal, with random imaginary parts in bins 0 and n_fft / 2 (the operator ignores them),
    and the same spectra with those imaginary parts 0"""
    wav = SH.make_signal(n_fft + hop * (T - 1), seed=7 * n_fft + hop + T, batch=rows)
    clean = SH.ref_stft64(wav, n_fft, hop, win, center=False).to(torch.complex64)
    g = torch.Generator().manual_seed(n_fft + T)
    dirty = clean.clone()
    dirty.imag[:, 0] = torch.randn(rows, T, generator=g)
    dirty.imag[:, -1] = torch.randn(rows, T, generator=g)
    return dirty, clean


def inverse_calls(n_fft, hop, T, center):
    """[(length, frame_counts)] of one (geometry, T, center): the default length (where a sample remains), default + 100 with a ragged batch"""
    default = max(n_fft + hop * (T - 1) - (2 * (n_fft // 2) if center else 0), 0)
    calls = [(default, None)] if default >= 1 else []
    return calls + [(default + 100, [T, T // 2, 1, 0])]


def inverse_refs(S, n_fft, hop, win, center, length, fc):
    """the float64 reference of one call and the yardstick error Y of its windowed frames"""
    out64, fr64, wss, ab, cnt = ref_istft_ola64(S, n_fft, hop, win, center, length, fc)
    Y = float(np.abs(inverse_yardstick32(S, n_fft, win, fc).double().numpy() - fr64).max())
    return dict(out=out64, frames=fr64, Y=Y, bound=inverse_bound(out64, wss, ab, cnt, Y))


def judge_inverse(ref, frames_got, out_got):
    """-> (frame error, worst share of the per-sample bound, samples that had to be exactly 0 and are not)"""
    e_fr = float(np.abs(np.asarray(frames_got, dtype=np.float64) - ref['frames']).max())
    err = np.abs(np.asarray(out_got, dtype=np.float64) - ref['out'])
    exact = ref['bound'] == 0
    share = float((err[~exact] / ref['bound'][~exact]).max()) if (~exact).any() else 0.0
    return e_fr, share, int((err[exact] != 0).sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# spectral subtraction
# ------------------------------------------------------------------------------------------------------------------------------------
SUBTRACT_GEOMS = [(512, 128, 512), (2048, 240, 1200)]


def soft_threshold64(S, v):
    S = torch.as_tensor(S).to(torch.complex128)
    mag = S.abs()
    pos = mag > 0
    return torch.where(pos, S * (torch.clamp(mag - v, min=0) / torch.where(pos, mag, torch.ones_like(mag))), torch.zeros_like(S))


def subtract_case(n_fft, hop, win):
    wav = SH.make_signal(66 * hop + 7, seed=n_fft + 1, batch=ROWS)
    want = SH.ref_stft64(wav, n_fft, hop, win)
    want.imag[:, 0] = 0
    want.imag[:, -1] = 0
    yard = cerr(SH.yardstick32(wav, n_fft, hop, win), want)
    mag = want.abs()
    return dict(wav=wav, want=want, yard=yard, vs=[0.0, 0.1, float(mag.median()), 2.0 * float(mag.max())])


def judge_subtract(got, case, v):
    """-> (worst share of the element-wise bound, elements that had to be exactly 0 and are not)"""
    want = case['want']
    ref = torch.view_as_real(soft_threshold64(want, v))
    g = torch.view_as_real(torch.as_tensor(got).to(torch.complex128).cpu())
    bnd = (2.0 * case['yard'] + 4.0 * U * want.abs())[..., None]
    share = float(((g - ref).abs() / bnd).max())
    must0 = (want.abs() < v - 2.0 * case['yard'])[..., None].expand_as(g)
    bad = int((g[must0] != 0).sum()) + int((g[:, 0, :, 1] != 0).sum()) + int((g[:, -1, :, 1] != 0).sum())
    return share, bad


def soft_threshold32(S, v):
    """the epilogue in float32 (bins 0 and n_fft / 2 are real)"""
    S = torch.as_tensor(S).to(torch.complex64).clone()
    S.imag[:, 0] = 0
    S.imag[:, -1] = 0
    m = torch.sqrt(S.real * S.real + S.imag * S.imag)
    sc = torch.where(m > 0, torch.clamp(m - np.float32(v), min=0) / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(m))
    return torch.complex(S.real * sc, S.imag * sc)


# ------------------------------------------------------------------------------------------------------------------------------------
# mel
# ------------------------------------------------------------------------------------------------------------------------------------
MEL_GEOMS = [(256, 64, 256), (512, 50, 240)]         # `red > lds` in dsv_logmel from M = 80 / from M = 33 on (asserted by the host test)
MEL_ROWS = (1, 33, 80, 128)


def dense_basis(M, n_fft):
    n_bins = n_fft // 2 + 1
    return (np.random.default_rng(M + n_fft).random((M, n_bins)) / n_bins).astype(np.float32)


def mel_signal(flavour, n_fft, hop, T):
    """(operator overrides, waveform): T frames exactly; one frame compares 64 rows, 65 frames compare 4.  The hifigan flavour's reflect
    padding (n_fft - hop) / 2 must stay below L, which at 512/50 (pad 231) forces four frames: its ONE-frame case overrides pad=0."""
    rows = ROWS if T > 2 else 64
    over = {}
    if flavour == 'pwg':
        L = hop * (T - 1) + hop - 1
    else:
        pad = (n_fft - hop) // 2
        L = n_fft - 2 * pad + hop * (T - 1)
        if L <= pad:                                  # reflect padding needs pad < L
            L = pad + 1
        if row_frames(L, n_fft, hop, pad, pad) != T:
            over, L = dict(pad=0), n_fft + hop * (T - 1)
    wav = SH.make_signal(L, seed=L + n_fft + T, batch=rows, noise=0.3) * (1.3 if flavour != 'pwg' else 1.0)
    return over, wav


def logmel_refs(wav, basis, flavour, over, n_fft, hop, win):
    """float64 (log-mel, linear mel, magnitude) [B][T][.] and the yardstick's errors in the log domain and on the magnitude: SH.ref_logmel64
    and SH.yardstick32 as they stand.  Overrides reach them as a flavour entry that exists only for the duration of these two calls."""
    key = flavour + ''.join(f'+{k}={v}' for k, v in sorted((over or {}).items()))
    with mock.patch.dict(SH.FLAVOURS, {key: dict(SH.FLAVOURS[flavour], **(over or {}))}):
        want, mel, mag = SH.ref_logmel64(wav, basis, key, n_fft, hop, win)
        y_log, _, y_mag = SH.yardstick32(wav, n_fft, hop, win, basis=basis, flavour=key)
    return dict(want=want, mel=mel, mag=mag, yard=float((y_log.double() - want).abs().max()), yard_mag=float((y_mag.double() - mag).abs().max()))


def onehot_bases(n_fft=256, M=128):
    """row m selects bin m / bin m + 1: together every bin 0 .. 128, Nyquist included"""
    n_bins = n_fft // 2 + 1
    a, b = np.zeros((M, n_bins), np.float32), np.zeros((M, n_bins), np.float32)
    a[np.arange(M), np.arange(M)] = 1.0
    b[np.arange(M), np.arange(M) + 1] = 1.0
    return [(a, 0), (b, 1)]


def onehot_ulps(out, lin, shift, floor, log10):
    """|out[..., m] - float32(log(float64(max(lin[..., m + shift], floor))))| in float32 ulps of the expected value, maximum"""
    lin = np.asarray(lin, dtype=np.float32)
    M = out.shape[-1]
    x = np.maximum(lin[..., shift:shift + M], np.float32(floor)).astype(np.float64)
    want = (np.log10(x) if log10 else np.log(x)).astype(np.float32)
    return float((np.abs(np.asarray(out, dtype=np.float32).astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


# ------------------------------------------------------------------------------------------------------------------------------------
# ragged rows
# ------------------------------------------------------------------------------------------------------------------------------------
def single_reflection64(x, length, pl, pr):
    """include/dsv.h, `lengths`: the padded signal of a row of `length` valid samples in reflect mode - ONE reflection about the row's own
    first / last sample, 0 where that leaves the row (a row no longer than its padding).  float64 [pl + length + pr]"""
    x = np.asarray(x, dtype=np.float64)
    u = np.arange(-pl, length + pr)
    v = np.where(u < 0, -u, np.where(u >= length, 2 * (length - 1) - u, u))
    ok = (v >= 0) & (v < length)
    return np.where(ok, x[np.where(ok, v, 0)], 0.0)


def ragged_reflect_case(n_fft=512, hop=128, win=512, L=1500, lens=(1500, 300, 256, 100, 2, 1)):
    """rows whose reflect padding (n_fft / 2 per side) reaches or passes their own length: per-row references, and ONE yardstick error for the
    case - the maximum over its rows (a row of one or two samples is no sample of the float32 contraction's error).  Such a row has its own
    condition instead (`tight`): its single frame is a sum of n <= 2 products x[i] basis[.][k], |basis| <= 1 - one rounding of the basis entry,
    one of the product, n - 1 of the sum (u = 2^-24, the unit roundoff): |err| <= gamma sum |x[i]|, gamma = (n + 1) u / (1 - (n + 1) u)."""
    pad = n_fft // 2
    wav = SH.make_signal(L, seed=77, batch=len(lens))
    refs, yards, tight = [], [], []
    for b, n in enumerate(lens):
        xp = single_reflection64(wav[b, :n].numpy(), n, pad, pad)
        want = SH.ref_stft64(torch.from_numpy(xp), n_fft, hop, win, center=False)
        yard = cerr(SH.yardstick32(torch.from_numpy(xp.astype(np.float32)), n_fft, hop, win, center=False), want)
        refs.append(want)
        yards.append(yard)
        gamma = (n + 1) * U / (1.0 - (n + 1) * U)                               # (1 + u)^(n + 1) - 1 <= gamma
        tight.append(gamma * float(wav[b, :n].double().abs().sum()) if n <= 2 else None)
    return dict(wav=wav, lens=list(lens), refs=refs, yard=max(yards), tight=tight, T=1 + L // hop)
