"""The optimisers of the vocoder training rows on the HIP operators of include/dsv.h, section "Vocoder optimisers" (kernels: csrc/voc_optim.hpp).

    MultiTensorOptimizer   a torch.optim.Optimizer whose update runs over the LIST of parameter tensors as they lie in memory: one set of
                           launches per (parameter group, step count) bucket instead of a Python loop of tensor operations per parameter
    RAdam                  modules/parallel_wavegan/optimizers/radam.py, the optimiser configs/tts/pwg.yaml configures, in its arithmetic
    AdamW                  torch.optim.AdamW (amsgrad off), dsf_adamw_step's arithmetic; HiFi-GAN: AdamW(params, lr, betas=(hp['adam_b1'], hp['adam_b2']))
    pwg_optimizers         (opt_g, opt_d, sched_g, sched_d) from the *_optimizer_params / *_scheduler_params blocks of configs/tts/pwg.yaml

State per parameter is the reference RAdam's: `step` a Python int, `exp_avg`, `exp_avg_sq`; a state_dict of either loads into the other, and
load_state_dict also takes torch.optim.AdamW's tensor `step`.  Being Optimizers, torch's schedulers (StepLR) and state_dict machinery work on
them unchanged.  Nothing here keeps a view of a gradient: the steps of pwg_train.py / hifigan_train.py set .grad to None before every backward
and their autograd nodes hand out fresh gradient tensors, which are read where they lie.

clip_and_step(max_norm) is clip_grad_norm_(params, max_norm) followed by step() WITHOUT a host synchronisation: dsv_mt_grad_norm leaves the
norm and the clip coefficient on the device and the update multiplies every gradient by that coefficient as it reads it.  It differs from the
torch pair in one respect: .grad is left UNSCALED (clip_grad_norm_ scales it in place); the update is the one of the scaled gradient.

float32 parameters on the device only; there is no CPU path, as elsewhere in this package."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

__all__ = ['MultiTensorOptimizer', 'RAdam', 'AdamW', 'pwg_optimizers', 'launch_count']

_LAUNCHES = [0]


def launch_count() -> int:
    """kernels launched through the library by this module since import"""
    return _LAUNCHES[0]


def _check(t, what):
    if not isinstance(t, torch.Tensor) or t.is_sparse or not t.is_cuda or t.dtype != torch.float32:
        kind = f'{t.dtype} on {t.device}' + (' (sparse)' if t.is_sparse else '') if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f'MultiTensorOptimizer: {what} must be a dense float32 tensor on the device, got {kind} (no CPU path)')


def _ptrs(tensors):
    """host array of the tensors' addresses"""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _counts(tensors):
    """host array of the tensors' element counts"""
    return (C.c_int64 * len(tensors))(*[t.numel() for t in tensors])


def _launches(lib, tensors, final=0):
    """launches one entry point makes for this list: the tables' capacity walked as csrc/voc_optim_abi.hpp walks it"""
    c, kt, kc = lib.dsv_mt_chunk_floats(), lib.dsv_mt_table_tensors(), lib.dsv_mt_table_chunks()
    n, nt, nc = 0, 0, 0
    for t in tensors:
        left = -(-t.numel() // c)
        while left:
            if nt == kt or nc == kc:
                n, nt, nc = n + 1, 0, 0
            take = min(left, kc - nc)
            nt, nc, left = nt + 1, nc + take, left - take
    return n + (1 if nc else 0) + final


class MultiTensorOptimizer(torch.optim.Optimizer):
    """Base of RAdam and AdamW: parameter groups of lr, betas, eps, weight_decay; _ENTRY names the subclass's entry point."""

    _ENTRY = None

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if self._ENTRY is None:
            raise TypeError('MultiTensorOptimizer is the base class: construct RAdam or AdamW')
        if not lr >= 0 or not eps >= 0 or not weight_decay >= 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f'{type(self).__name__}: bad hyper-parameters (lr={lr} betas={tuple(betas)} eps={eps} weight_decay={weight_decay})')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    def load_state_dict(self, state_dict):
        """torch's, then `step` as a Python int (torch.optim.AdamW keeps a tensor) and dense float32 moments"""
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            if not st:
                continue
            st['step'] = int(st['step'].item()) if isinstance(st['step'], torch.Tensor) else int(st['step'])
            for k in ('exp_avg', 'exp_avg_sq'):
                st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()

    def _buckets(self):
        """[(group, step after this update, [p], [g], [m], [v])]: the parameters that have a gradient, by (group, step count), in group order"""
        out = []
        for group in self.param_groups:
            by_step = {}
            for p in group['params']:
                if p.grad is None:
                    continue
                _check(p, 'a parameter')
                _check(p.grad, 'a gradient')
                if p.grad.device != p.device:
                    raise RuntimeError('MultiTensorOptimizer: a gradient lives on another device than its parameter')
                if not p.is_contiguous():
                    raise RuntimeError('MultiTensorOptimizer: a parameter must be contiguous (it is updated where it lies)')
                st = self.state[p]
                if not st:
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                ps, gs, ms, vs = by_step.setdefault(st['step'] + 1, ([], [], [], []))
                ps.append(p)
                gs.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                ms.append(st['exp_avg'])
                vs.append(st['exp_avg_sq'])
            out += [(group, step) + lists for step, lists in sorted(by_step.items())]
        return out

    def _update(self, buckets, gscale):
        lib = _lib.load()
        fn = getattr(lib, self._ENTRY)
        for group, step, ps, gs, ms, vs in buckets:
            dev = ps[0].device
            if any(p.device != dev for p in ps):
                raise RuntimeError('MultiTensorOptimizer: the parameters of one group must live on one device')
            if gscale is not None and gscale.device != dev:
                raise RuntimeError('MultiTensorOptimizer: clip_and_step needs every parameter on one device')
            pa, ga, ma, va, na = _ptrs(ps), _ptrs(gs), _ptrs(ms), _ptrs(vs), _counts(ps)
            b1, b2 = group['betas']
            with torch.cuda.device(dev):
                _lib.check(fn(pa, ga, ma, va, na, len(ps), float(group['lr']), float(b1), float(b2), float(group['eps']), float(group['weight_decay']),
                              step, _lib.ptr(gscale), torch.cuda.current_stream(dev).cuda_stream), self._ENTRY)
            _LAUNCHES[0] += _launches(lib, ps)
            for p in ps:
                self.state[p]['step'] = step

    @torch.no_grad()
    def step(self, closure=None):
        """one update of every parameter that has a gradient; a parameter without one is skipped and its step count does not advance"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._update(self._buckets(), None)
        return loss

    @torch.no_grad()
    def clip_and_step(self, max_norm):
        """clip_grad_norm_(every parameter of this optimiser, max_norm) + step() with no host synchronisation.  -> the norm before clipping, a
        0-dim device tensor.  .grad is NOT scaled (see the module docstring)."""
        lib = _lib.load()
        self._opt_called = True                                # what a scheduler's wrapper of step() records: this IS a step (no order warning)
        buckets = self._buckets()
        if not buckets:
            p0 = self.param_groups[0]['params'][0]
            return torch.zeros((), device=p0.device, dtype=torch.float32)
        grads = [g for b in buckets for g in b[3]]
        dev = grads[0].device
        if any(g.device != dev for g in grads):
            raise RuntimeError('MultiTensorOptimizer: clip_and_step needs every parameter on one device')
        ga, na = _ptrs(grads), _counts(grads)
        nws = lib.dsv_mt_workspace_floats(na, len(grads))
        ws = torch.empty(nws // 2, device=dev, dtype=torch.float64)
        out2 = torch.empty(2, device=dev, dtype=torch.float32)
        _lib.call('dsv_mt_grad_norm', dev, ga, na, len(grads), float(max_norm), ws.data_ptr(), nws, out2.data_ptr())
        _LAUNCHES[0] += _launches(lib, grads, final=1)
        self._update(buckets, out2[1:])
        return out2[0]


class RAdam(MultiTensorOptimizer):
    """Rectified Adam as modules/parallel_wavegan/optimizers/radam.py steps it (dsv_mt_radam_step): the variance rectification switches on
    where N_sma >= 5 - from step 6 on with beta2 = 0.999 or 0.99; before that the update is the bias-corrected momentum alone."""
    _ENTRY = 'dsv_mt_radam_step'


class AdamW(MultiTensorOptimizer):
    """torch.optim.AdamW, amsgrad off (dsv_mt_adamw_step); weight_decay defaults to torch's 0.01."""
    _ENTRY = 'dsv_mt_adamw_step'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


def pwg_optimizers(gen, disc, hp):
    """The ParallelWaveGAN trainer's optimisers and schedulers from configs/tts/pwg.yaml: RAdam(**hp['generator_optimizer_params']) on the
    generator with StepLR(**hp['generator_scheduler_params']), the same from the discriminator's two blocks.
    -> (opt_g, opt_d, sched_g, sched_d); call sched.step() once per training step, after the optimiser's."""
    opt_g = RAdam([p for p in gen.parameters() if p.requires_grad], **hp['generator_optimizer_params'])
    opt_d = RAdam([p for p in disc.parameters() if p.requires_grad], **hp['discriminator_optimizer_params'])
    sched_g = torch.optim.lr_scheduler.StepLR(opt_g, **hp['generator_scheduler_params'])
    sched_d = torch.optim.lr_scheduler.StepLR(opt_d, **hp['discriminator_scheduler_params'])
    return opt_g, opt_d, sched_g, sched_d
