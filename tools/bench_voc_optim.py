"""Developer tool (GPU): the vocoder optimisers of diffsinger_amd/voc_optim.py (clip_and_step: global-norm clip + update, RAdam and AdamW) on two
real parameter sets - the weight-normed ParallelWaveGAN generator's (several hundred small tensors) and MultiPeriodDiscriminator's (about 41 M
elements in 90 tensors) - beside, in the same process on the same gradients:

    torch_foreach     torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True)
    dsf_loop          clip_grad_norm_ + one dsf_adamw_step per tensor (the flat-range kernel of the FastSpeech2 row, in a Python loop)

Events around `iters` steps, best of three windows (tools/bench_pe_train.py's timing).  One JSON line per parameter set: ms per step, kernel
launches per step, and for the HIP optimisers the bytes the update moves (28 B per element: p, g, m, v read, p, m, v written) over the time,
with its fraction of the 8 TB/s HBM peak.  The norm's read of g (4 B per element more) is not counted: the figure is a lower bound.

    python tools/bench_voc_optim.py [iters]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffsinger_amd import _lib, voc_optim

HBM_PEAK = 8.0e12
HP = dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
MAX_NORM = 10.0


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
        return len([e for e in prof.events() if e.device_type.name == 'CUDA' and 'Memcpy' not in e.name and 'Memset' not in e.name])
    except Exception as e:                      # the profiler is optional here
        return f'n/a ({type(e).__name__})'


def clones(params):
    out = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for q, p in zip(out, params):
        q.grad = p.grad.clone()
    return out


def bench(name, module, iters):
    dev = torch.device('cuda', 0)
    params = [p for p in module.to(dev).parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 0.01
    n = sum(p.numel() for p in params)
    row = {'parameters': name, 'tensors': len(params), 'elements': n, 'max_norm': MAX_NORM}
    for kind in ('RAdam', 'AdamW'):
        ps = clones(params)
        opt = getattr(voc_optim, kind)(ps, **HP)
        step = lambda: opt.clip_and_step(MAX_NORM)
        step()
        before = voc_optim.launch_count()
        step()
        row[f'hip_{kind.lower()}_launches'] = voc_optim.launch_count() - before
        ms = time_ms(step, iters)
        row[f'hip_{kind.lower()}_ms'] = round(ms, 4)
        row[f'hip_{kind.lower()}_GBps'] = round(28.0 * n / (ms * 1e-3) / 1e9, 1)
        row[f'hip_{kind.lower()}_hbm_fraction'] = round(28.0 * n / (ms * 1e-3) / HBM_PEAK, 4)
    # torch: clip_grad_norm_ scales .grad in place, so the gradients are restored from a copy inside the timed step of BOTH baselines alike
    ps = clones(params)
    saved = [p.grad.clone() for p in ps]
    topt = torch.optim.AdamW(ps, foreach=True, **HP)

    def restore():
        torch._foreach_copy_([p.grad for p in ps], saved)

    def torch_step():
        restore()
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=True)
        topt.step()
    restore_ms = time_ms(restore, iters)
    row['torch_foreach_ms'] = round(time_ms(torch_step, iters) - restore_ms, 4)
    row['torch_foreach_launches'] = launches(torch_step)
    lib = _lib.load()
    ps2 = clones(params)
    saved2 = [p.grad.clone() for p in ps2]
    ms_, vs_ = [torch.zeros_like(p) for p in ps2], [torch.zeros_like(p) for p in ps2]
    count = [0]

    def restore2():
        torch._foreach_copy_([p.grad for p in ps2], saved2)

    def loop_step():
        restore2()
        torch.nn.utils.clip_grad_norm_(ps2, MAX_NORM, foreach=True)
        count[0] += 1
        s = torch.cuda.current_stream(dev).cuda_stream
        for p, m, v in zip(ps2, ms_, vs_):
            _lib.check(lib.dsf_adamw_step(p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), HP['lr'], HP['betas'][0], HP['betas'][1],
                                          HP['eps'], HP['weight_decay'], count[0], None, s), 'dsf_adamw_step')
    row['dsf_loop_ms'] = round(time_ms(loop_step, iters) - time_ms(restore2, iters), 4)
    row['dsf_loop_launches'] = launches(loop_step)
    row['restore_ms_subtracted'] = round(restore_ms, 4)
    print(json.dumps(row), flush=True)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    from diffsinger_amd import MultiPeriodDiscriminator
    from diffsinger_amd.pwg import ParallelWaveGANGenerator
    torch.manual_seed(1234)
    bench('ParallelWaveGANGenerator (30 layers, weight norm)', ParallelWaveGANGenerator(), iters)
    bench('MultiPeriodDiscriminator', MultiPeriodDiscriminator(), iters)


if __name__ == '__main__':
    main()
