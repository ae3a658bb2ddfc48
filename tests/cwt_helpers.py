"""Shared plumbing of the CWT pitch tests (csrc/fs2_cwt.hpp; tests/test_cwt_host.py, tests/test_gpu_cwt.py): float64 restatements of
FastSpeech2.cwt2f0_norm (modules/fastspeech/fs2.py:239-245 with utils/cwt.py:118-147 and utils/pitch_utils.py:34-42) and of the cwt branch of
FastSpeech2Task.add_pitch_loss (tasks/tts/fs2.py:233-267), the case tables, seeded operands, and the writer of tests/golden/cwt_pitch.npz:

    python -m tests.cwt_helpers          # rewrites the fixture from the reference tree (a child process runs the reference's own functions)

TEST INFRASTRUCTURE ONLY.  The fixture holds data: fp32 inputs and the float64 results of the reference's functions on them."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cwt_pitch.npz')
HEADER = os.path.join(ROOT, 'diffsinger_amd', 'csrc', 'fs2_cwt.hpp')
F64, F32 = torch.float64, torch.float32
SCALES = 10
HP_NORM = {'log': dict(pitch_norm='log'), 'standard': dict(pitch_norm='standard', f0_mean=214.0, f0_std=63.5)}
ROW_MEANS = (6.0, 7.5, 6.7)             # log-f0 means of the rows: 400 Hz beside 1800 Hz in one batch


def header_constant(name):
    return int(re.search(r'constexpr int ' + name + r' = (\d+);', open(HEADER).read()).group(1))


BLOCK = header_constant('kCwtBlock')            # 256: threads of every kernel of fs2_cwt.hpp, the stride of a row's frame loop
LOSS_BLOCKS = header_constant('kCwtLossBlocks')  # 256: partial blocks of the loss before its grid-stride loop wraps
LOSS_BWD_BLOCKS = 1024                          # the cap of k_cwt_loss_bwd's grid (dsf_cwt_pitch_loss_bwd)


# ----------------------------------------------------------------------------------------------------------------------------------------
# float64 restatements (any dtype really: the dtype of the operands)
# ----------------------------------------------------------------------------------------------------------------------------------------
def scale_weights(like):
    """utils/cwt.py:120: (arange.float() + 1 + 2.5) ** -2.5 - fp32 values in the reference whatever the dtype of cwt_spec."""
    return ((torch.arange(0, SCALES).float()[None, None, :] + 1 + 2.5) ** (-2.5)).to(device=like.device, dtype=like.dtype)


def cwt2f0_norm_ref(cwt_spec, mean, std, T_out, hp, std_scale=1.0, live=None, frozen_stats=False):
    """cwt2f0 + the repeat of the last frame up to T_out columns + norm_f0; live (an int): the statistics over the first `live` frames only -
    the frame_keep variant of diffsinger_amd/fs2.py's cwt2f0_norm (mean and unbiased deviation of the live frames, z for every frame).
    frozen_stats: the same values, but no gradient through the row statistics (the size of the terms that cancel in d cwt: error_rule)."""
    rec = (cwt_spec * scale_weights(cwt_spec)).sum(-1)
    T = rec.shape[1]
    sel = rec if (live is None or int(live) == T) else rec[:, :int(live)]
    mu, sigma = sel.mean(-1, keepdim=True), sel.std(-1, keepdim=True)
    if frozen_stats:
        mu, sigma = mu.detach(), sigma.detach()
    z = (rec - mu) / sigma
    f0 = (z * (std * std_scale)[:, None] + mean[:, None]).exp()
    f0 = torch.cat([f0] + [f0[:, -1:]] * (T_out - T), 1)
    if hp['pitch_norm'] == 'standard':
        return (f0 - hp['f0_mean']) / hp['f0_std']
    return torch.log2(f0)


def cwt2f0_norm_today(cwt_spec, mean, std, T_out, hp, fk=None):
    """The torch expression FastSpeech2.cwt2f0_norm runs where the operator does not (diffsinger_amd/fs2.py), verbatim, in the operands' dtype:
    the yardstick whose fp32 error the operator's error is judged by.  fk = (keep [B,T], live scalar tensor) as frame_keep returns them."""
    b = (torch.arange(0, 10, device=cwt_spec.device).float()[None, None, :] + 1 + 2.5) ** (-2.5)
    rec = (cwt_spec * b).sum(-1)
    full = (rec - rec.mean(-1, keepdim=True)) / rec.std(-1, keepdim=True)
    if fk is None:
        rec = full
    else:
        keep, live = fk
        mu = (rec * keep).sum(-1, keepdim=True) / live
        dev = (rec - mu) * keep
        masked = (rec - mu) / ((dev * dev).sum(-1, keepdim=True) / (live - 1)).sqrt()
        rec = torch.where(live == rec.shape[1], full, masked)
    f0 = (rec * std[:, None] + mean[:, None]).exp()
    f0 = torch.cat([f0] + [f0[:, -1:]] * (T_out - f0.shape[1]), 1)
    if hp['pitch_norm'] == 'standard':
        return (f0 - hp['f0_mean']) / hp['f0_std']
    return torch.log2(f0)


def pitch_loss_ref(output, sample, hp):
    """The cwt branch of add_pitch_loss (+ add_f0_loss under cwt_add_f0_loss) in the dtype of the operands: the reference's keys, in its order."""
    L = collections.OrderedDict()
    mel2ph, f0, uv = sample['mel2ph'], sample.get('f0'), sample.get('uv')
    nonpadding = (mel2ph != 0).to(output['cwt'].dtype)
    cwt_pred = output['cwt'][:, :, :10]
    fn = F.l1_loss if hp['cwt_loss'] == 'l1' else F.mse_loss
    L['C'] = fn(cwt_pred, sample['cwt_spec']) * hp['lambda_f0']
    if hp['use_uv']:
        assert output['cwt'].shape[-1] == 11
        L['uv'] = (F.binary_cross_entropy_with_logits(output['cwt'][:, :, -1], uv, reduction='none') * nonpadding).sum() / nonpadding.sum() * hp['lambda_uv']
    L['f0_mean'] = F.l1_loss(output['f0_mean'], sample['f0_mean']) * hp['lambda_f0']
    L['f0_std'] = F.l1_loss(output['f0_std'], sample['f0_std']) * hp['lambda_f0']
    if hp.get('cwt_add_f0_loss'):
        assert not hp['use_uv'], 'the reference indexes channel 1 of a one-channel tensor there (tasks/tts/fs2.py:257)'
        f0_cwt = cwt2f0_norm_ref(cwt_pred, output['f0_mean'], output['f0_std'], mel2ph.shape[1], hp)
        pf = F.l1_loss if hp['pitch_loss'] == 'l1' else F.mse_loss
        L['f0'] = (pf(f0_cwt, f0, reduction='none') * nonpadding).sum() / nonpadding.sum() * hp['lambda_f0']
    return L


# ----------------------------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------------------------
FwdCase = collections.namedtuple('FwdCase', 'B T pad live layout norm std_scale')       # pad = T_out - T; live: frames of the statistics
LossCase = collections.namedtuple('LossCase', 'B T loss use_uv layout mask')

# frame counts: the small ones, around a wave (64), and around the kernel's block size kCwtBlock = 256 (one frame per thread and pass): one
# short of it, at it, one past it, and twice that plus one (a thread's third frame)
FWD_T = (2, 3, 33, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
FWD_PAD = (0, 1, 7)
LAYOUTS = ('view11', 'contig')          # cwt as [:, :, :10] of an 11-wide tensor / a contiguous 10-wide one


def fwd_cases():
    """Every T x pad x live at B = 3 and B = 1, with layout / pitch_norm / std_scale rotating so that each value of each meets every T, and
    the full cross of layout x norm x std_scale x live at T = 65.  live is one of T, T - 1, 2.
    LEFT OUT, because the reference itself is non-finite there (a division by a zero deviation): live = 1 (T = 2 with live = T - 1) and
    constant rows.  Nothing else is."""
    out = []
    i = 0
    for B in (3, 1):
        for T in FWD_T:
            for pad in FWD_PAD:
                for live in sorted({T, T - 1, 2}):
                    if live < 2:
                        continue
                    out.append(FwdCase(B, T, pad, live, LAYOUTS[i % 2], ('log', 'standard')[(i // 2) % 2], (1.0, 0.8)[(i // 4) % 2]))
                    i += 1
            i += 1                          # shift the rotation from one T to the next
    for layout in LAYOUTS:
        for norm in ('log', 'standard'):
            for sc in (1.0, 0.8):
                for live in (65, 64, 2):
                    out.append(FwdCase(3, 65, 7, live, layout, norm, sc))
    return list(dict.fromkeys(out))


def loss_cases():
    """l1 / l2 x use_uv x layout x mask at small T; the block seams of the partial sums (B * T around kCwtBlock); one case past
    kCwtLossBlocks * kCwtBlock frames (the forward's grid-stride loop wraps) and one past 1024 * kCwtBlock (the backward's does).
    mask: 'ragged' rows of different lengths, 'one_live' a row with exactly one live frame, 'row_padded' a row that is padding throughout."""
    out = []
    for loss in ('l1', 'l2'):
        for use_uv in (True, False):
            for layout in LAYOUTS:
                for mask in ('ragged', 'one_live', 'row_padded'):
                    out.append(LossCase(3, 33, loss, use_uv, layout, mask))
    for T in (2, BLOCK - 1, BLOCK, BLOCK + 1):
        out.append(LossCase(1, T, 'l1', True, 'view11', 'ragged'))
    out.append(LossCase(3, 85, 'l2', True, 'view11', 'ragged'))                                  # B * T = 255
    out.append(LossCase(3, LOSS_BLOCKS * BLOCK // 3 + 1, 'l1', True, 'view11', 'ragged'))         # 65538 frames: > 256 blocks of 256
    out.append(LossCase(3, LOSS_BWD_BLOCKS * BLOCK // 3 + 1, 'l2', True, 'contig', 'ragged'))     # 262146 frames: > 1024 blocks of 256
    return out


def _layout(t, layout, g):
    """[B,T,10] scales -> the parent the operator is given ([B,T,11] with a random last channel, or the tensor itself) and the 10-wide view."""
    if layout == 'contig':
        return t, t
    parent = torch.cat([t, torch.randn(t.shape[0], t.shape[1], 1, generator=g)], 2).contiguous()
    return parent, parent[:, :, :10]


def mel2ph_for(B, T_out, live, g):
    """[B, T_out] int64: row 0 owns the first `live` frames, the later rows fewer; no row owns a column behind `live`."""
    m = torch.zeros(B, T_out, dtype=torch.int64)
    for b in range(B):
        n = live if b == 0 else max(1, live - 1 - int(torch.randint(0, max(live // 2, 1), (1,), generator=g)))
        m[b, :n] = torch.randint(1, 9, (n,), generator=g).sort().values
    return m


def case_seed(c):
    """A seed that does not depend on Python's string hashing."""
    s = 0
    for v in c:
        for ch in str(v):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def fwd_operands(c, seed=None):
    """fp32, on the CPU: parent (what holds the scales), mean / std [B], mel2ph [B, T_out] whose last owned column is live - 1."""
    g = torch.Generator().manual_seed(1000 + (case_seed(c) if seed is None else seed))
    scales = torch.randn(c.B, c.T, SCALES, generator=g)              # standard normal; a constant row has probability zero
    parent, _ = _layout(scales, c.layout, g)
    mean = torch.tensor(ROW_MEANS[:c.B]) if c.B > 1 else torch.tensor([ROW_MEANS[(c.T + c.pad) % 2]])
    std = torch.rand(c.B, generator=g) * 0.5 + 0.1                   # [0.1, 0.6]
    return dict(parent=parent, mean=mean, std=std, mel2ph=mel2ph_for(c.B, c.T + c.pad, c.live, g))


def loss_operands(c):
    g = torch.Generator().manual_seed(2000 + case_seed(c))
    B, T = c.B, c.T
    scales = torch.randn(B, T, SCALES, generator=g)
    if c.use_uv:
        parent = torch.cat([scales, torch.randn(B, T, 1, generator=g) * 2], 2)
        parent[B - 1, T - 1, 10], parent[0, 0, 10], parent[0, 1, 10] = 30.0, 30.0, -30.0        # the stable BCE form: exp(-|x|), not exp(x)
        if c.layout == 'view11':
            wide = torch.randn(B, T, 13, generator=g)
            wide[:, :, :11] = parent
            parent = wide[:, :, :11]                                      # an 11-wide view of a 13-wide tensor: every stride but the last differs
        else:
            parent = parent.contiguous()
    else:
        if c.layout == 'view11':
            parent = torch.cat([scales, torch.randn(B, T, 1, generator=g)], 2)[:, :, :10]      # 10 channels on an 11-wide tensor
        else:
            parent = scales
    mel2ph = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        n = T if b == 0 else max(1, T - 1 - (5 * b) % T)
        if c.mask == 'one_live' and b == B - 1:
            n = 1
        if c.mask == 'row_padded' and b == B - 1:
            n = 0
        mel2ph[b, :n] = torch.randint(1, 9, (n,), generator=g).sort().values
    uv = (torch.rand(B, T, generator=g) < 0.3).float()
    uv[0, 0], uv[0, 1 % T] = 0.0, 1.0                                     # logit +30 against 0, -30 against 1: the two large BCE values
    f0 = (torch.rand(B, T, generator=g) * 2 + 7.5) * (mel2ph > 0)
    return dict(cwt=parent, cwt_spec=torch.randn(B, T, SCALES, generator=g), uv=uv, mel2ph=mel2ph, f0=f0,
                f0_mean=torch.rand(B, generator=g) * 1.5 + 6.0, f0_std=torch.rand(B, generator=g) * 0.5 + 0.1,
                f0_mean_pred=torch.rand(B, generator=g) * 1.5 + 6.0, f0_std_pred=torch.rand(B, generator=g) * 0.5 + 0.1)


def loss_hp(c, **kw):
    return dict(dict(pitch_type='cwt', cwt_loss=c.loss, use_uv=c.use_uv, lambda_f0=0.7, lambda_uv=1.3, pitch_loss='l1', cwt_add_f0_loss=False,
                     pitch_norm='log'), **kw)


REF_NOISE = 2.0 ** -40     # see error_rule


def error_rule(got, ref64, today32, cancelling=None):
    """(ratio, error, allowance): the operator's distance from float64 against max(2 x the torch fp32 expression's own distance, 4 ulp of the
    largest reference value) - the floor covers the exp, the log2 and two roundings; the factor 2 a different order of summation.
    cancelling: a float64 tensor of the size of the terms whose difference the reference value is.  With two frames in the statistics z is
    +-1/sqrt(2) whatever the scales are, so d cwt is identically zero: the float64 reference then holds its own rounding (1e-16 of terms
    of size ~1), the fp32 expression may hold an exact 0, and the rule would compare one evaluation's rounding with another's.  The
    reference's own error, 2^-40 of those terms (1e-12: a thousand times the float64 rounding, a hundred thousand times below fp32's), is
    therefore allowed too; it matters in no other case."""
    ref64 = ref64.to(F64)
    err = float((got.to(F64) - ref64).abs().max()) if got.numel() else 0.0
    e_ref = float((today32.to(F64) - ref64).abs().max()) if got.numel() else 0.0
    allow = max(2 * e_ref, 4 * 2.0 ** -23 * float(ref64.abs().max()) if got.numel() else 0.0)
    if cancelling is not None:
        allow = max(allow, REF_NOISE * float(cancelling.abs().max()))
    ratio = err / allow if allow > 0 else (0.0 if err == 0 else float('inf'))
    return ratio, err, allow


# ----------------------------------------------------------------------------------------------------------------------------------------
# the golden fixture: the reference's own functions on the CPU, float64
# ----------------------------------------------------------------------------------------------------------------------------------------
GOLDEN_FWD = (FwdCase(3, 65, 7, 65, 'view11', 'log', 1.0), FwdCase(2, 33, 0, 33, 'contig', 'standard', 1.0), FwdCase(1, 2, 1, 2, 'view11', 'log', 1.0))
GOLDEN_LOSS = ((LossCase(3, 33, 'l1', True, 'view11', 'ragged'), {}), (LossCase(2, 70, 'l2', True, 'contig', 'one_live'), {}),
               (LossCase(3, 17, 'l1', False, 'contig', 'ragged'), dict(cwt_add_f0_loss=True, pitch_loss='l1')),
               (LossCase(2, 40, 'l2', False, 'view11', 'ragged'), dict(cwt_add_f0_loss=True, pitch_loss='l2', pitch_norm='standard', f0_mean=214.0, f0_std=63.5)))

# the third-party modules the reference's task modules import and this machine lacks: none is used by the functions run here
_ABSENT = ('h5py', 'librosa', 'parselmouth', 'pycwt', 'pyloudnorm', 'pytorch_lightning', 'skimage', 'webrtcvad')

_CHILD = r'''
import importlib.abc, importlib.machinery, importlib.util, os, sys, types
sys.dont_write_bytecode = True
sys.path.insert(0, %(root)r)
import numpy as np, torch
import scipy.signal, scipy.signal.windows
if not hasattr(scipy.signal, 'kaiser'):
    scipy.signal.kaiser = scipy.signal.windows.kaiser            # layers/pqmf.py:12 imports the pre-1.13 name
class Stub(types.ModuleType):
    __path__ = []
    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        return type(k, (), {})
class Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    roots = set(n for n in %(absent)r if importlib.util.find_spec(n) is None)
    def find_spec(self, name, path, target=None):
        if name.split('.')[0] in self.roots:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
    def create_module(self, spec):
        return Stub(spec.name)
    def exec_module(self, m):
        pass
sys.meta_path.insert(0, Finder())
from tests import cwt_helpers as H
sys.path.insert(0, %(ref)r)
os.chdir(%(ref)r)
from utils.hparams import hparams
from modules.fastspeech.fs2 import FastSpeech2
from tasks.tts.fs2 import FastSpeech2Task
out = {}
hparams['cwt_scales'] = np.arange(10)                              # only its length is used (utils/cwt.py:118-125)
for i, c in enumerate(H.GOLDEN_FWD):
    o = H.fwd_operands(c, seed=i)
    hparams.update(H.HP_NORM[c.norm], use_uv=True)
    scales = o['parent'][:, :, :10].double()
    got = FastSpeech2.cwt2f0_norm(None, scales, o['mean'].double(), o['std'].double(), o['mel2ph'])
    out.update({f'fwd{i}_parent': o['parent'].numpy(), f'fwd{i}_mean': o['mean'].numpy(), f'fwd{i}_std': o['std'].numpy(),
                f'fwd{i}_mel2ph': o['mel2ph'].numpy(), f'fwd{i}_out': got.numpy()})
for i, (c, kw) in enumerate(H.GOLDEN_LOSS):
    o = H.loss_operands(c)
    hp = H.loss_hp(c, **kw)
    hparams.update(hp)
    task = types.SimpleNamespace()
    task.cwt_loss = lambda p, g: FastSpeech2Task.cwt_loss(task, p, g)
    task.add_f0_loss = lambda *a, **k: FastSpeech2Task.add_f0_loss(task, *a, **k)
    task.model = types.SimpleNamespace(cwt2f0_norm=lambda *a: FastSpeech2.cwt2f0_norm(None, *a))
    d = lambda t: t.double() if t.is_floating_point() else t
    output = {'cwt': d(o['cwt']), 'f0_mean': d(o['f0_mean_pred']), 'f0_std': d(o['f0_std_pred'])}
    sample = {k: d(o[k]) for k in ('cwt_spec', 'uv', 'mel2ph', 'f0', 'f0_mean', 'f0_std')}
    losses = {}
    FastSpeech2Task.add_pitch_loss(task, output, sample, losses)
    for k in ('cwt', 'cwt_spec', 'uv', 'mel2ph', 'f0', 'f0_mean', 'f0_std', 'f0_mean_pred', 'f0_std_pred'):
        out[f'loss{i}_{k}'] = o[k].contiguous().numpy()
    out[f'loss{i}_keys'] = np.array(list(losses))
    out[f'loss{i}_values'] = np.array([float(v) for v in losses.values()], dtype=np.float64)
np.savez_compressed(%(dst)r, **out)
print('CWT_REFERENCE_OK', len(out))
'''


def run_reference(dst):
    """Run the reference's cwt2f0_norm / add_pitch_loss on the GOLDEN_* cases in a child process (its modules shadow `utils`, `tasks`) -> dst (npz)."""
    from oracle.ref_driver import REFERENCE_ROOT
    res = subprocess.run([sys.executable, '-c', _CHILD % dict(root=ROOT, ref=REFERENCE_ROOT, absent=_ABSENT, dst=dst)], capture_output=True, text=True)
    assert 'CWT_REFERENCE_OK' in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    return dict(np.load(dst))


def load_golden():
    return dict(np.load(GOLDEN))


def golden_fwd(g, i):
    """-> (case, operands as tensors, the reference's float64 output)"""
    c = GOLDEN_FWD[i]
    o = {k: torch.from_numpy(g[f'fwd{i}_{k}']) for k in ('parent', 'mean', 'std', 'mel2ph')}
    return c, o, torch.from_numpy(g[f'fwd{i}_out'])


def golden_loss(g, i):
    c, kw = GOLDEN_LOSS[i]
    o = {k: torch.from_numpy(g[f'loss{i}_{k}']) for k in ('cwt', 'cwt_spec', 'uv', 'mel2ph', 'f0', 'f0_mean', 'f0_std', 'f0_mean_pred', 'f0_std_pred')}
    return c, loss_hp(c, **kw), o, [str(k) for k in g[f'loss{i}_keys']], torch.from_numpy(g[f'loss{i}_values'])


def restate_loss(o, hp, dtype=F64):
    """pitch_loss_ref on the operands of loss_operands / golden_loss in `dtype` -> OrderedDict"""
    d = lambda t: t.to(dtype) if t.is_floating_point() else t
    output = {'cwt': d(o['cwt']), 'f0_mean': d(o['f0_mean_pred']), 'f0_std': d(o['f0_std_pred'])}
    sample = {k: d(o[k]) for k in ('cwt_spec', 'uv', 'mel2ph', 'f0', 'f0_mean', 'f0_std')}
    return pitch_loss_ref(output, sample, hp)


if __name__ == '__main__':
    print(GOLDEN, len(run_reference(GOLDEN)), 'arrays,', os.path.getsize(GOLDEN), 'bytes')
