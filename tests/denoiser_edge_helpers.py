"""Test infrastructure of the denoiser's edge tests (tests/test_denoiser_edges_host.py, tests/test_gpu_denoiser_edges.py).  CPU only: nothing
here touches the HIP library.

  layer / forward     the oracle's residual layer and network (oracle/diffnet_oracle.py residual_layer, diffnet_forward; usr/diff/net.py:66-78,
                      :107-130) restated in the dtype of the parameters handed in, with the 3-tap dilated convolution behind a hook
                      conv(y, w, b, d).  conv=None is F.conv1d: in float32 the same bits as the oracle, in float64 the yardstick's reference.
  wino_conv32         the convolution as Winograd F(2,3) along the frame axis, as csrc/dsd_loop_wino.hpp lines 7-10 state it: the float32 CPU
                      form of what k_loop_wino_sa, k_lat_conv_w and the training stack's Winograd kernels sum.
  tolerance           the bound of a device tensor: 4 x the error of the float32 CPU form of the same sums against float64, on the test's own
                      inputs, never below 16 u max|ref| and never above the flat figure the suite used before.
  mutant_a / _b / _c  three wrong convolutions at the granularity the kernels work at (32-frame tiles, the utterances of a batch adjacent in the
                      tile list): what a broken tail, halo or tile seam computes.  The host test shows that the bound catches each of them.

Lengths: for d in {1, 2, 4, 8} the lengths 1, d, d+1, 2d, 2d+1 (an outer tap never meets the signal; a Winograd pair (t, t + d) straddles the
end), 32-d, 32, 33, 32+d (the d frames next to a tile boundary with and without a tile behind it), 64, 65 (two full tiles; an odd number of
tiles on the 64-frame kernel)."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import diffnet_oracle as O
from tests import helpers as H

PRESET = 'opencpop_ds60_rel'                    # dilation cycle 4: layers 0-3 are d = 1, 2, 4, 8; layer 19 is the last (skips only)
LAYERS = (0, 1, 2, 3, 19)
DILATIONS = (1, 2, 4, 8)
LENGTHS = sorted({T for d in DILATIONS for T in (1, d, d + 1, 2 * d, 2 * d + 1, 32 - d, 32, 33, 32 + d, 64, 65)})
SHORT = [1, 9, 32, 33, 65]
B = 3                                           # the middle utterance has a neighbour on both sides
TILE = 32
U = 2.0 ** -24                                  # unit roundoff of float32
FACTOR = 4.0
CAPS = {'layer': 2e-5, 'eval': 1e-5, 'mel': 1e-4, 'plms': 1e-4}      # the flat tolerances of the suite: nothing becomes looser than it was

assert LENGTHS == [1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 28, 30, 31, 32, 33, 34, 36, 40, 64, 65]


# ----------------------------------------------------------------------------------------------------------------------------------------
# model, inputs
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model():
    """(cfg, float32 oracle parameters, their float64 copy, preset) of PRESET"""
    pre = H.presets()[PRESET]
    cfg = H.net_config(pre)
    p32 = H.oracle_params(cfg)
    p64 = {k: v.double() for k, v in p32.items()}
    assert [cfg.dilation(l) for l in LAYERS] == [1, 2, 4, 8, 8]
    return cfg, p32, p64, pre


@functools.lru_cache(maxsize=None)
def inputs(T, batch=B, n_noise=0):
    """Seeded float32 inputs of length T: x [B,256,T] (a layer's input), spec [B,1,80,T] (the network's), cond [B,256,T] as a view of [B,T,256]
    (what the reference hands the denoiser), one step index for the whole batch (t0) and one per utterance (t)."""
    g = torch.Generator().manual_seed(52000 + 131 * T + batch)
    out = dict(x=torch.randn(batch, 256, T, generator=g), cond=torch.randn(batch, T, 256, generator=g).transpose(1, 2),
               spec=torch.randn(batch, 1, 80, T, generator=g), t0=(7 * T + 37) % 100,
               t=torch.tensor([(13 * b + 29 * T + 5) % 100 for b in range(batch)]))
    if n_noise:
        out['noise'] = torch.randn(n_noise, batch, 1, 80, T, generator=g)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# the layer and the network, convolution behind a hook
# ----------------------------------------------------------------------------------------------------------------------------------------
def layer(p, cfg, l, x, cond, d_emb, conv=None):
    """oracle.diffnet_oracle.residual_layer in the dtype of p -> (x_out, skip).  conv(y, w, b, d) replaces the dilated convolution; a hook with
    the attribute needs_dp also receives the step projection dp [B,C,1] (what a tail that is not zeroed holds)."""
    pre = f'residual_layers.{l}.'
    dt = p[pre + 'dilated_conv.weight'].dtype
    x, cond, d_emb = x.to(dt), cond.to(dt), d_emb.to(dt)
    dil = cfg.dilation(l)
    dp = F.linear(d_emb, p[pre + 'diffusion_projection.weight'], p[pre + 'diffusion_projection.bias']).unsqueeze(-1)
    cp = F.conv1d(cond, p[pre + 'conditioner_projection.weight'], p[pre + 'conditioner_projection.bias'])
    y = x + dp
    w, b = p[pre + 'dilated_conv.weight'], p[pre + 'dilated_conv.bias']
    if conv is None:
        y = F.conv1d(y, w, b, padding=dil, dilation=dil) + cp
    elif getattr(conv, 'needs_dp', False):
        y = conv(y, w, b, dil, dp) + cp
    else:
        y = conv(y, w, b, dil) + cp
    gate, filt = torch.chunk(y, 2, dim=1)
    y = torch.sigmoid(gate) * torch.tanh(filt)
    y = F.conv1d(y, p[pre + 'output_projection.weight'], p[pre + 'output_projection.bias'])
    res, skip = torch.chunk(y, 2, dim=1)
    return (x + res) / math.sqrt(2.0), skip


def forward(p, cfg, spec, t, cond, conv=None):
    """oracle.diffnet_oracle.diffnet_forward in the dtype of p, composed of `layer`.  spec [B,1,M,T], t [B] -> eps_hat [B,1,M,T]."""
    dt = p['input_projection.weight'].dtype
    x = F.relu(F.conv1d(spec[:, 0].to(dt), p['input_projection.weight'], p['input_projection.bias']))
    d_emb = O.step_mlp(p, cfg, t)
    skips = []
    for l in range(cfg.residual_layers):
        x, s = layer(p, cfg, l, x, cond, d_emb, conv)
        skips.append(s)
    x = torch.sum(torch.stack(skips), dim=0) / math.sqrt(cfg.residual_layers)
    x = F.relu(F.conv1d(x, p['skip_projection.weight'], p['skip_projection.bias']))
    x = F.conv1d(x, p['output_projection.weight'], p['output_projection.bias'])
    return x[:, None, :, :]


def wino_conv32(y, w, b, d):
    """The 3-tap convolution of dilation d as Winograd F(2,3) over the frame pairs (t, t + d), in the dtype of y (float32: the yardstick of the
    Winograd kernels; float64: equal to F.conv1d up to rounding).  y [B,C,T], w [Co,C,3], b [Co] -> [B,Co,T].

    Frame t is the even frame of its pair iff (t // d) % 2 == 0.  With d0 = y[t-d], d1 = y[t], d2 = y[t+d], d3 = y[t+2d] (zero outside [0, T)):
        M0 = g0 (d0 - d2)    M1 = U1 (d1 + d2)    M2 = U2 (d2 - d1)    M3 = g2 (d3 - d1)        out[t] = (M1 + M2) + M0    out[t+d] = (M1 - M2) + M3
    U1 = (g0 + g1 + g2) / 2 and U2 = (g0 - g1 + g2) / 2 are float64 sums rounded once (k_pack_wino); each operand is one add in y's dtype."""
    Bn, Cc, T = y.shape
    dt = y.dtype
    nblk = (T + 2 * d - 1) // (2 * d)
    yp = F.pad(y, (0, nblk * 2 * d - T)).reshape(Bn, Cc, nblk, 2, d)
    E, Od = yp[:, :, :, 0], yp[:, :, :, 1]                             # [B,C,nblk,d]: y[tE], y[tE + d]
    zero = torch.zeros_like(E[:, :, :1])
    Oprev = torch.cat((zero, Od[:, :, :-1]), dim=2)                    # y[tE - d]
    Enext = torch.cat((E[:, :, 1:], zero), dim=2)                      # y[tE + 2d]
    g = w.double()
    U = [w[:, :, 0], ((g[:, :, 0] + g[:, :, 1] + g[:, :, 2]) / 2).to(dt), ((g[:, :, 0] - g[:, :, 1] + g[:, :, 2]) / 2).to(dt), w[:, :, 2]]
    ops = [Oprev - Od, E + Od, Od - E, Enext - E]
    M = [F.conv1d(a.reshape(Bn, Cc, nblk * d), u.to(dt)[:, :, None]).reshape(Bn, -1, nblk, d) for a, u in zip(ops, U)]
    out = torch.stack(((M[1] + M[2]) + M[0], (M[1] - M[2]) + M[3]), dim=3)          # [B,Co,nblk,2,d]
    return out.reshape(Bn, -1, nblk * 2 * d)[:, :, :T] + b.to(dt)[None, :, None]


# ----------------------------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------------------------
def maxerr(a, ref64):
    return float((torch.as_tensor(a).double().cpu() - ref64).abs().max())


def tolerance(kind, ref64, yard32):
    """The bound of one device tensor against its float64 value ref64: FACTOR x the error of yard32 - the float32 CPU form of the same sums on
    the same inputs (the oracle for a direct-form kernel, the wino_conv32 form for a Winograd kernel) - with the floor 16 u max|ref64| and the
    cap CAPS[kind] ('plms': relative to max(1, max|ref64|), the mel of that sampler is not clamped).  The reference sets it, not the kernel."""
    top = float(ref64.abs().max())
    cap = CAPS[kind] * (max(1.0, top) if kind == 'plms' else 1.0)
    return min(cap, max(FACTOR * maxerr(yard32, ref64), 16 * U * top))


def report(label, got, bound, yard=None):
    """One printed line per comparison: measured maximum, bound, share used (and the device / yardstick ratio)."""
    tail = '' if yard is None else f', {got / max(yard, 1e-30):.2f} x the yardstick\'s {yard:.3e}'
    print(f'{label}: max {got:.3e}, bound {bound:.3e}, share {got / bound:.2f}{tail}')
    return got / bound


# ----------------------------------------------------------------------------------------------------------------------------------------
# references, computed once per length
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_refs(T):
    """{layer: dict(ref=(x_out64, skip64), direct=(..32), wino=(..32))} on inputs(T), skip WITHOUT the out-projection's skip bias (the kernels
    add the skip biases once, in the head)."""
    cfg, p32, p64, _ = model()
    inp = inputs(T)
    out = {}
    with torch.no_grad():
        d_emb = O.step_mlp(p32, cfg, torch.full((B,), inp['t0']))
        for l in LAYERS:
            bias = p32[f'residual_layers.{l}.output_projection.bias'][256:, None]
            r = {'ref': layer(p64, cfg, l, inp['x'], inp['cond'], d_emb), 'direct': layer(p32, cfg, l, inp['x'], inp['cond'], d_emb),
                 'wino': layer(p32, cfg, l, inp['x'], inp['cond'], d_emb, conv=wino_conv32)}
            out[l] = {k: (xo, sk - bias.to(sk.dtype)) for k, (xo, sk) in r.items()}
    return out


@functools.lru_cache(maxsize=None)
def eval_refs(T):
    """dict(ref=eps64, direct=eps32, wino=eps32) of one evaluation with a step per utterance on inputs(T)"""
    cfg, p32, p64, _ = model()
    inp = inputs(T)
    with torch.no_grad():
        return {'ref': forward(p64, cfg, inp['spec'], inp['t'], inp['cond']), 'direct': forward(p32, cfg, inp['spec'], inp['t'], inp['cond']),
                'wino': forward(p32, cfg, inp['spec'], inp['t'], inp['cond'], conv=wino_conv32)}


def schedule():
    """(float32 schedule tables, spec_min, spec_max) of PRESET"""
    _, _, _, pre = model()
    smin = torch.tensor(pre['spec_min'], dtype=torch.float32)[None, None, :]
    smax = torch.tensor(pre['spec_max'], dtype=torch.float32)[None, None, :]
    return O.make_schedule(H.betas_for(pre)), smin, smax


def mel_refs(kind, cond, x_T, noise=None, k_step=3, interval=0):
    """(mel64, mel32) of O.infer_mel: the sampler in float64 (the float32 schedule tables, inputs and weights, every sum in double) and the
    float32 oracle run that is the yardstick.  'plms' row by row: the reference's PLMS is B = 1."""
    cfg, p32, p64, _ = model()
    sch, smin, smax = schedule()
    res = []
    for p, dt in ((p64, torch.float64), (p32, torch.float32)):
        s = {k: v.to(dt) for k, v in sch.items()}
        c, x, lo, hi = cond.to(dt), x_T.to(dt), smin.to(dt), smax.to(dt)
        if kind == 'plms':
            res.append(torch.cat([O.infer_mel(p, cfg, s, c[b:b + 1], lo, hi, k_step=k_step, x_T=x[b:b + 1], pndm_interval=interval)
                                  for b in range(x.shape[0])]))
        else:
            res.append(O.infer_mel(p, cfg, s, c, lo, hi, k_step=k_step, noises=list(noise.to(dt)), x_T=x))
    return res[0], res[1]


DDPM_K, PLMS_K, PLMS_INTERVAL = 3, 100, 25      # K = 3 ancestral steps with explicit noise; PLMS 100 / 25: four iterations, five evaluations


@functools.lru_cache(maxsize=None)
def loop_refs(kind, T):
    """(mel64, mel32) of the K-step loop `kind` ('ddpm' / 'plms') from x_T = inputs(T)['spec']"""
    inp = inputs(T, n_noise=DDPM_K)
    if kind == 'ddpm':
        return mel_refs('ddpm', inp['cond'], inp['spec'], inp['noise'], k_step=DDPM_K)
    return mel_refs('plms', inp['cond'], inp['spec'], k_step=PLMS_K, interval=PLMS_INTERVAL)


# ----------------------------------------------------------------------------------------------------------------------------------------
# mutants: three wrong convolutions at tile granularity
# ----------------------------------------------------------------------------------------------------------------------------------------
def _tiled_conv(y, w, b, d, dp=None, foreign_halo=False, drop_left_at_seam=False):
    """The convolution the way the kernels walk it: every utterance padded to whole 32-frame tiles, the tiles of the batch in one list, a tap
    that leaves its tile read from the neighbouring tile of the list.  With the three switches off this IS F.conv1d (the host test checks it)."""
    Bn, Cc, T = y.shape
    TS = (T + TILE - 1) // TILE * TILE
    yp = F.pad(y, (0, TS - T))
    if dp is not None:                                                  # (a) the tail behind T holds x + dp = dp instead of zero
        yp[:, :, T:] = dp.to(y.dtype)
    flat = yp.permute(1, 0, 2).reshape(Cc, Bn * TS)                     # the tile list: utterances adjacent
    left = F.pad(flat, (d, 0))[:, :Bn * TS]                             # y[t - d]
    right = F.pad(flat, (0, d))[:, d:]                                  # y[t + d]
    pos = torch.arange(Bn * TS) % TS
    if not foreign_halo:                                                # (b) the halo of an utterance's first / last tile comes from the neighbour
        left = left * (pos >= d)
        right = right * (pos < TS - d)
    if drop_left_at_seam:                                               # (c) the left tap of the first d frames of a tile is lost
        left = left * ((pos % TILE >= d) | (pos < TILE))
    out = sum(F.conv1d(v[None], w[:, :, k, None]) for k, v in enumerate((left, flat, right)))[0] + b[:, None]
    return out.reshape(-1, Bn, TS).permute(1, 0, 2)[:, :, :T]


def tiled_conv(y, w, b, d):
    return _tiled_conv(y, w, b, d)


def mutant_a(y, w, b, d, dp):
    """the tail of y = x + step projection is not zeroed behind T: observable at every length that is no multiple of 32"""
    return _tiled_conv(y, w, b, d, dp=dp)
mutant_a.needs_dp = True


def mutant_b(y, w, b, d):
    """the halo of an utterance's outer tiles is taken from the neighbouring utterance: observable iff T > 32 ceil(T / 32) - d"""
    return _tiled_conv(y, w, b, d, foreign_halo=True)


def mutant_c(y, w, b, d):
    """the left tap is dropped across a tile boundary inside an utterance: observable iff T > 32"""
    return _tiled_conv(y, w, b, d, drop_left_at_seam=True)


MUTANTS = {'a': (mutant_a, lambda T, d: T % TILE != 0),
           'b': (mutant_b, lambda T, d: T > (T + TILE - 1) // TILE * TILE - d),
           'c': (mutant_c, lambda T, d: T > TILE)}
