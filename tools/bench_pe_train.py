"""Developer tool (GPU): one training step of the HIP PitchExtractor (PitchExtractionTask: forward in train mode + pitch loss + backward, dropout
0.1 on) at 8 x 1024 mel frames, hidden_size 256, beside the same operator sequence in PyTorch eager (MIOpen / ATen kernels, torch autograd) on the
same GPU and the same parameters.  One JSON line: ms per step and kernel launches per step of both.      python tools/bench_pe_train.py [iters]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import diffsinger_amd
from diffsinger_amd import hparams


def eager_step(p, mel, f0, uv, hp, pos_table, drop=0.1):
    """The operator sequence of the training step as torch ops on [B,C,T] tensors (p: the module's parameters / buffers by name)."""
    keep = 1 - mel.abs().sum(-1).eq(0).float()[:, None, :]
    x = mel.transpose(1, 2)
    for l in range(3):
        k = f'mel_prenet.layers.{l}.'
        x = F.relu(F.conv1d(x, p[k + '0.weight'], p[k + '0.bias'], padding=2))
        x = F.batch_norm(x, p[k + '2.running_mean'], p[k + '2.running_var'], p[k + '2.weight'], p[k + '2.bias'], True, 0.1, 1e-5) * keep
    x = F.linear(x.transpose(1, 2), p['mel_prenet.out_proj.weight'], p['mel_prenet.out_proj.bias']) * keep.transpose(1, 2)
    x = F.linear(x, p['mel_encoder.in_proj.weight'], p['mel_encoder.in_proj.bias']).transpose(1, 2)
    for i in range(2):
        k = f'mel_encoder.conv.{i}.'
        w = p[k + 'conv.conv.weight']
        x = x + F.relu(F.group_norm(F.conv1d(x, w, p[k + 'conv.conv.bias'], padding=2), w.shape[0] // 16, p[k + 'norm.weight'], p[k + 'norm.bias'], 1e-5))
    x = F.linear(x.transpose(1, 2), p['mel_encoder.out_proj.weight'], p['mel_encoder.out_proj.bias'])
    nz = x[..., 0].ne(0).int()
    pos = (torch.cumsum(nz, 1) * nz).long()
    x = x + p['pitch_predictor.pos_embed_alpha'] * pos_table.index_select(0, pos.view(-1)).view(x.shape)
    x = x.transpose(1, 2)
    kk = hp['predictor_kernel']
    for i in range(5):
        k = f'pitch_predictor.conv.{i}.'
        x = F.relu(F.conv1d(F.pad(x, [(kk - 1) // 2, (kk - 1) // 2]), p[k + '1.weight'], p[k + '1.bias']))
        x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), p[k + '3.weight'], p[k + '3.bias'], 1e-12).transpose(1, 2)
        x = F.dropout(x, drop, True)
    pred = F.linear(x.transpose(1, 2), p['pitch_predictor.linear.weight'], p['pitch_predictor.linear.bias'])
    nonpadding = (mel.abs().sum(-1) > 0).float()
    loss = (F.binary_cross_entropy_with_logits(pred[:, :, 1], uv, reduction='none') * nonpadding).sum() / nonpadding.sum() * hp['lambda_uv']
    nonpadding = nonpadding * (uv == 0).float()
    loss = loss + (F.l1_loss(pred[:, :, 0], f0, reduction='none') * nonpadding).sum() / nonpadding.sum() * hp['lambda_f0']
    loss.backward()
    return loss


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type.name == 'CUDA' and 'Memcpy' not in e.name and 'Memset' not in e.name]
        top = {}
        for e in prof.events():
            if e.device_type.name == 'CUDA' and 'Memcpy' not in e.name and 'Memset' not in e.name:
                top[e.name[:60]] = top.get(e.name[:60], 0.0) + e.device_time
        return len(names), sorted(((round(v / 1e3, 3), k) for k, v in top.items()), reverse=True)[:6]
    except Exception as e:                      # the profiler is optional here
        return f'n/a ({type(e).__name__})', []


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    hparams.clear()
    diffsinger_amd.use_preset('opencpop_ds1000')
    hp = dict(pitch_loss='l1', use_uv=True, lambda_f0=1.0, lambda_uv=1.0, predictor_kernel=hparams['predictor_kernel'])
    hp.update({k: hparams[k] for k in ('pitch_loss', 'use_uv', 'lambda_f0', 'lambda_uv') if k in hparams})
    from diffsinger_amd.pe import PitchExtractor, pe_training_step
    torch.manual_seed(1234)
    dev = torch.device('cuda', 0)
    m = PitchExtractor().to(dev).train()
    B, T = 8, 1024
    mel = torch.randn(B, T, 80, device=dev) * 1.5 - 4
    for b in range(1, B):
        mel[b, T - 20 * b:] = 0
    f0 = 7.5 + 0.5 * torch.randn(B, T, device=dev)
    uv = (torch.rand(B, T, device=dev) < 0.3).float()
    sample = {'mels': mel, 'f0': f0, 'uv': uv}

    def hip_step():
        for q in m.parameters():
            q.grad = None
        total, _ = pe_training_step(m, sample, hp)
        total.backward()
        return total

    p = {k: v.detach().clone().requires_grad_(v.is_floating_point() and 'running' not in k and '_float_tensor' not in k) for k, v in m.state_dict().items()}
    pos_table = m.pitch_predictor.embed_positions.table(T).to(dev)

    def torch_step():
        for q in p.values():
            q.grad = None
        return eager_step(p, mel, f0, uv, hp, pos_table)

    lh, lt = float(hip_step().detach()), float(torch_step().detach())
    n_hip, top_hip = launches(hip_step)
    n_torch, top_torch = launches(torch_step)
    row = {'model': 'PitchExtractor training step (forward + loss + backward, dropout 0.1)', 'B': B, 'T_mel': T, 'hidden_size': hparams['hidden_size'],
           'hip_ms': round(time_ms(hip_step, iters), 4), 'torch_eager_ms': round(time_ms(torch_step, iters), 4), 'hip_launches': n_hip,
           'torch_launches': n_torch, 'loss_hip': lh, 'loss_torch': lt, 'hip_top_kernels_ms': top_hip, 'torch_top_kernels_ms': top_torch}
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
