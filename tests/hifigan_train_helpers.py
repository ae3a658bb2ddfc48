"""Test infrastructure of HiFi-GAN generator training (groundwork: the HIP training path is not built): the generator restated on explicit
tensors in any dtype on any device (differentiable; written from modules/hifigan/hifigan.py:30-92, 104-169 and
modules/parallel_wavegan/models/source.py:518-531, independent of the product code), the float64 operator functions with the bounds a device
backward is to be held to, and the fixture.

THE RULE, the tolerances and the weight-norm bounds are those of tests/pwg_train_helpers.py (RULE = 16 u, u = 2^-24; margin 4 over the float32
reference error with the floor RULE max|grad|): they are imported, not re-chosen.

THE MASKS.  A leaky ReLU's derivative jumps at zero.  Float32 and float64 evaluations of the same network disagree on the sign of a handful of
the 10^5 .. 10^6 leaky-ReLU inputs (|x| ~ 1e-7), and one flipped sign moves whole gradient tensors by thousands of times the rule.  `generator`
therefore takes `masks`, one bool tensor per leaky ReLU in call order: where given, lrelu(x) = where(mask, x, slope x) - the derivative is the
mask's, whatever the sign of this evaluation's x.  Whole-module comparisons evaluate float64 on the masks of the float32 side being judged and
cap the number of flips separately.  With masks and sine_waves omitted the restatement equals oracle.hifigan_oracle.generator bitwise in
float32 on the CPU."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.pwg_train_helpers import RULE, U, d64, mse_to, tolerances, weight_norm_bounds  # noqa: F401  (re-exported)

LRELU_SLOPE, POST_SLOPE = 0.1, 0.01
FIXTURE_CFG = dict(resblock='1', upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4], upsample_initial_channel=32,
                   resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, audio_sample_rate=24000)


def config(use_pitch_embed=False, **over):
    h = dict(FIXTURE_CFG, use_pitch_embed=bool(use_pitch_embed))
    h.update(over)
    return h


def get_padding(k, d=1):
    return int((k * d - d) / 2)


def hop_of(h):
    return int(np.prod(h['upsample_rates']))


def block_dils(h, j):
    d = tuple(h['resblock_dilation_sizes'][j])
    return d[:3] if str(h['resblock']) == '1' else d[:2]


def module_prefixes(h):
    """parameter holders in forward order: (prefix, weight shape, weight-normed)"""
    c0, rates, ksz = h['upsample_initial_channel'], h['upsample_rates'], h['upsample_kernel_sizes']
    out = [('conv_pre.', (c0, 80, 7), True)]
    if h['use_pitch_embed']:
        out.append(('m_source.l_linear.', (1, 9), False))
    ch = c0
    for i, (u, k) in enumerate(zip(rates, ksz)):
        ch = c0 // 2 ** (i + 1)
        out.append((f'ups.{i}.', (2 * ch, ch, k), True))
        if h['use_pitch_embed']:
            s = int(np.prod(rates[i + 1:])) if i + 1 < len(rates) else 0
            out.append((f'noise_convs.{i}.', (ch, 1, 2 * s if s else 1), False))
    nk = len(h['resblock_kernel_sizes'])
    for i in range(len(rates)):
        ch = c0 // 2 ** (i + 1)
        for j, k in enumerate(h['resblock_kernel_sizes']):
            p = f'resblocks.{i * nk + j}.'
            for q in range(len(block_dils(h, j))):
                out += [(f'{p}convs1.{q}.', (ch, ch, k), True), (f'{p}convs2.{q}.', (ch, ch, k), True)] if str(h['resblock']) == '1' else [
                    (f'{p}convs.{q}.', (ch, ch, k), True)]
    return out + [('conv_post.', (1, ch, 7), True)]


def module_shapes(h, weight_norm_on=True):
    out = {}
    for p, shp, wn in module_prefixes(h):
        out[p + 'bias'] = (shp[1] if p.startswith('ups.') else shp[0],)
        if wn and weight_norm_on:
            out[p + 'weight_g'] = (shp[0],) + (1,) * (len(shp) - 1)
            out[p + 'weight_v'] = shp
        else:
            out[p + 'weight'] = shp
    return out


def synth_state(shapes, seed):
    """A seeded O(1) state (pwg_train_helpers.synth_state's recipe; a transposed convolution's fan-in counts the taps that reach one output
    sample): weight_v ~ N(0, 1 / fan_in), weight_g so that every OUTPUT channel sees unit-scale rows, biases 0.1 N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    st = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith('bias'):
            st[k] = 0.1 * torch.randn(shp, generator=gen)
        elif k.endswith('weight_g'):
            st[k] = 0.7 + 0.6 * torch.rand(shp, generator=gen)
        elif k.endswith('weight_v') or k.startswith('m_source') or k.startswith('noise_convs'):
            st[k] = torch.randn(shp, generator=gen) / float(np.prod(shp[1:])) ** 0.5
        else:
            w = torch.randn(shp, generator=gen)
            gsh = (shp[0],) + (1,) * (len(shp) - 1)
            st[k] = (0.7 + 0.6 * torch.rand(gsh, generator=gen)) * w / w.flatten(1).norm(dim=1).reshape(gsh)
    for k in st:                              # ups: weight_norm's rows are INPUT channels with Co * k entries, of which k / u reach one output sample
        if k.startswith('ups.') and k.endswith('weight_g'):
            st[k] = st[k] * 2.0
    return st


def plain_weights(leaves, h):
    """{prefix + 'weight' / 'bias'} from a state in weight-normed or plain form; the weight-norm expression is torch's own op (what the oracle
    applies), differentiable in any dtype"""
    plain = {}
    for p, _, wn in module_prefixes(h):
        if p + 'weight' in leaves:
            plain[p + 'weight'] = leaves[p + 'weight']
        else:
            plain[p + 'weight'] = torch._weight_norm(leaves[p + 'weight_v'], leaves[p + 'weight_g'], 0)
        plain[p + 'bias'] = leaves[p + 'bias']
    return plain


class _Acts:
    """the leaky ReLUs of one evaluation in call order: records every input, applies the given masks"""

    def __init__(self, masks):
        self.masks, self.pre = masks, []

    def __call__(self, x, slope):
        self.pre.append(x)
        if self.masks is None:
            return F.leaky_relu(x, slope)
        m = self.masks[len(self.pre) - 1].to(x.device)
        assert m.shape == x.shape and m.dtype == torch.bool
        return torch.where(m, x, slope * x)


def generator(plain, h, x, f0=None, *, masks=None, sine_waves=None):
    """HifiGanGenerator.forward on a dict of plain weights -> (y, pre-activations in call order, sine_waves or None, har or None).  f0 given and
    sine_waves omitted: the oracle's SineGen on the CPU in float32 with the draws of torch's global generator in the reference's order."""
    rates, ksz = h['upsample_rates'], h['upsample_kernel_sizes']
    nk = len(h['resblock_kernel_sizes'])
    act = _Acts(masks)
    har = None
    if f0 is not None:
        if sine_waves is None:
            from oracle import hifigan_oracle as O
            f0u = F.interpolate(f0.detach().to('cpu', torch.float32)[:, None], scale_factor=float(hop_of(h)), mode='nearest').transpose(1, 2)
            sine_waves, uv = O.sine_gen(f0u, h['audio_sample_rate'])
            torch.randn_like(uv)
        sine_waves = sine_waves.to(x.device, x.dtype)
        har = torch.tanh(F.linear(sine_waves, plain['m_source.l_linear.weight'], plain['m_source.l_linear.bias'])).transpose(1, 2)
    x = F.conv1d(x, plain['conv_pre.weight'], plain['conv_pre.bias'], padding=3)
    for i, (u, k) in enumerate(zip(rates, ksz)):
        x = act(x, LRELU_SLOPE)
        x = F.conv_transpose1d(x, plain[f'ups.{i}.weight'], plain[f'ups.{i}.bias'], stride=u, padding=(k - u) // 2)
        if har is not None:
            if i + 1 < len(rates):
                s = int(np.prod(rates[i + 1:]))
                xs = F.conv1d(har, plain[f'noise_convs.{i}.weight'], plain[f'noise_convs.{i}.bias'], stride=s, padding=s // 2)
            else:
                xs = F.conv1d(har, plain[f'noise_convs.{i}.weight'], plain[f'noise_convs.{i}.bias'])
            x = x + xs
        acc = None
        for j in range(nk):
            p, kk = f'resblocks.{i * nk + j}.', h['resblock_kernel_sizes'][j]
            y = x
            for q, d in enumerate(block_dils(h, j)):
                if str(h['resblock']) == '1':
                    xt = act(y, LRELU_SLOPE)
                    xt = F.conv1d(xt, plain[f'{p}convs1.{q}.weight'], plain[f'{p}convs1.{q}.bias'], padding=get_padding(kk, d), dilation=d)
                    xt = act(xt, LRELU_SLOPE)
                    xt = F.conv1d(xt, plain[f'{p}convs2.{q}.weight'], plain[f'{p}convs2.{q}.bias'], padding=get_padding(kk, 1))
                else:
                    xt = act(y, LRELU_SLOPE)
                    xt = F.conv1d(xt, plain[f'{p}convs.{q}.weight'], plain[f'{p}convs.{q}.bias'], padding=get_padding(kk, d), dilation=d)
                y = xt + y
            acc = y if acc is None else acc + y
        x = acc / nk
    x = act(x, POST_SLOPE)
    x = F.conv1d(x, plain['conv_post.weight'], plain['conv_post.bias'], padding=3)
    return torch.tanh(x), act.pre, sine_waves, har


def masks_of(pre):
    """the derivative choice of the forward: x > 0 (a zero takes the slope)"""
    return [(t.detach() > 0).cpu() for t in pre]


def count_flips(masks_a, masks_b):
    """-> (number of leaky-ReLU inputs whose mask differs, number of inputs)"""
    assert len(masks_a) == len(masks_b)
    return sum(int((a.cpu() != b.cpu()).sum()) for a, b in zip(masks_a, masks_b)), sum(a.numel() for a in masks_a)


def module_grads(state, h, x, f0, loss_of, dtype=torch.float64, device='cpu', masks=None, sine_waves=None):
    """The module's output and the gradient of loss_of(output) with respect to every tensor of `state` (weight-normed or plain form), by autograd
    over the restatement in `dtype` on `device`.  -> (out, grads {key: tensor or None}, dw {prefix: gradient of the plain weight or None},
    pre-activations (detached), sine_waves)"""
    leaves = {k: v.detach().to(device, dtype).clone().requires_grad_(True) for k, v in state.items()}
    plain = plain_weights(leaves, h)
    for p, _, _ in module_prefixes(h):
        if p + 'weight' not in leaves:
            plain[p + 'weight'].retain_grad()
    f0d = None if f0 is None else f0.detach().to(device, dtype)
    out, pre, sw, _ = generator(plain, h, x.detach().to(device, dtype), f0d, masks=masks, sine_waves=sine_waves)
    loss_of(out).backward()
    grads = {k: (None if v.grad is None else v.grad.detach()) for k, v in leaves.items()}
    dw = {p: (None if plain[p + 'weight'].grad is None else plain[p + 'weight'].grad.detach()) for p, _, _ in module_prefixes(h)}
    return out.detach(), grads, dw, [t.detach() for t in pre], (None if sw is None else sw.detach())


# ---- operators with their bounds (float64, exact operands) -----------------------------------------------------------------------------------
def lrelu(x, slope):
    return torch.where(x > 0, x, slope * x)


def conv_wgrad(g, x, K, dil, pad, slope):
    """dw[o][i][k] = sum g[b][o][t] lrelu(x[b][i][t + k dil - pad]) -> (dw, bound), (db, bound)"""
    L = x.shape[2]
    a = F.pad(lrelu(x, slope), (pad, (K - 1) * dil - pad))
    dw = torch.stack([torch.einsum('bot,bit->oi', g, a[:, :, k * dil:k * dil + L]) for k in range(K)], 2)
    bw = torch.stack([torch.einsum('bot,bit->oi', g.abs(), a[:, :, k * dil:k * dil + L].abs()) for k in range(K)], 2)
    return (dw, RULE * bw), (g.sum((0, 2)), RULE * g.abs().sum((0, 2)))


def conv_dgrad(g, w, x_saved, dil, pad, slope, residual=None, sum_in=None, divide=1.0):
    """dx[b][i][t] = (m sum_o sum_k w[o][i][k] g[b][o][t - k dil + pad] + residual + sum_in) / divide, m = x_saved > 0 ? 1 : slope -> (dx, bound)"""
    K, L = w.shape[2], g.shape[2]
    gp = F.pad(g, ((K - 1) * dil - pad, pad))
    v = sum(torch.einsum('oi,bot->bit', w[:, :, k], gp[:, :, (K - 1 - k) * dil:(K - 1 - k) * dil + L]) for k in range(K))
    b = sum(torch.einsum('oi,bot->bit', w[:, :, k].abs(), gp[:, :, (K - 1 - k) * dil:(K - 1 - k) * dil + L].abs()) for k in range(K))
    if x_saved is not None:
        m = torch.where(x_saved > 0, torch.ones_like(x_saved), torch.full_like(x_saved, slope))
        v, b = v * m, b * m
    for extra in (residual, sum_in):
        if extra is not None:
            v, b = v + extra, b + extra.abs()
    return v / divide, RULE * b / divide


def _autograd_pair(fn, inputs, g):
    """gradients of fn(*inputs) under the cotangent g, and the same with every tensor replaced by its absolute value (the sums of |term|)"""
    def run(ins, gg):
        with torch.enable_grad():                                           # (callable from inside another node's backward)
            ins = [t.detach().clone().requires_grad_(True) for t in ins]
            return torch.autograd.grad(fn(*ins), ins, gg)
    return run(inputs, g), run([t.abs() for t in inputs], g.abs())


def conv_transpose_backward(g, x_saved, w, u, slope):
    """ConvTranspose1d(stride u, padding (k - u) / 2) behind a leaky ReLU, by float64 autograd -> (dx, bound), (dw, bound), (db, bound)"""
    k = w.shape[2]
    a = lrelu(x_saved, slope)
    m = torch.where(x_saved > 0, torch.ones_like(x_saved), torch.full_like(x_saved, slope))
    (da, dw), (ba, bw) = _autograd_pair(lambda a_, w_: F.conv_transpose1d(a_, w_, stride=u, padding=(k - u) // 2), [a, w], g)
    return (da * m, RULE * ba * m), (dw, RULE * bw), (g.sum((0, 2)), RULE * g.abs().sum((0, 2)))


def noise_conv_backward(g, har, w, s, pad):
    """Conv1d(1 -> C, K, stride s, padding pad) on har [B][L] -> (dw [C][K], bound), (db, bound), (dhar [B][L], bound)"""
    (dh, dw), (bh, bw) = _autograd_pair(lambda h_, w_: F.conv1d(h_[:, None], w_[:, None], stride=s, padding=pad), [har, w], g)
    return (dw, RULE * bw), (g.sum((0, 2)), RULE * g.abs().sum((0, 2))), (dh, RULE * bh)


def source_backward(dhar, har, sine_waves):
    """har = tanh(l_linear(sine_waves)): d weight [H], d bias [1] from the gradient at har, with their bounds"""
    dp = dhar * (1 - har * har)
    return (torch.einsum('bl,blh->h', dp, sine_waves), RULE * torch.einsum('bl,blh->h', dp.abs(), sine_waves.abs())), (
        dp.sum().reshape(1), RULE * dp.abs().sum().reshape(1))


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hifigan_train_ref.npz')
CASES = ('plain', 'nsf')


def pack_masks(masks):
    return np.packbits(np.concatenate([m.numpy().reshape(-1) for m in masks]))


def unpack_masks(bits, shapes):
    n = sum(int(np.prod(s)) for s in shapes)
    flat = torch.from_numpy(np.unpackbits(bits)[:n].astype(bool))
    out, o = [], 0
    for s in shapes:
        m = int(np.prod(s))
        out.append(flat[o:o + m].reshape(tuple(s)))
        o += m
    return out


def fixture(case):
    """tests/golden/hifigan_train_ref.npz (tools/make_golden_hifigan_train.py), case 'plain' or 'nsf' -> dict(h, state, x, f0, seed, target, out,
    grads, none_keys, masks, sine_waves, err, err_out); the state is stored as float16 (synth_state rounded by the tool) and returned as float32"""
    z = np.load(FIXTURE)
    pre = case + '/'
    meta = json.loads(str(z[pre + 'meta_json']))
    get = lambda k: torch.from_numpy(z[pre + k]) if pre + k in z.files else None                                                      # noqa: E731
    keys, shapes = meta['keys'], [tuple(s) for s in meta['shapes']]
    gkeys = [k for k in keys if k not in meta['none_keys']]

    def split(flat, ks):
        out, o = {}, 0
        for k in ks:
            shp = shapes[keys.index(k)]
            n = int(np.prod(shp))
            out[k] = torch.from_numpy(flat[o:o + n].astype(np.float32)).reshape(shp)
            o += n
        assert o == flat.size
        return out
    return dict(h=meta['h'], none_keys=meta['none_keys'], seed=meta['seed'], state=split(z[pre + 'state'], keys), grads=split(z[pre + 'grads'], gkeys),
                err=dict(zip(gkeys, (float(v) for v in z[pre + 'err']))), err_out=float(z[pre + 'err_out']), x=get('x'), f0=get('f0'),
                target=get('target'), out=get('out'), sine_waves=get('sine_waves'), masks=unpack_masks(z[pre + 'masks'], meta['mask_shapes']))
