"""Training dropout of FastSpeech2 on HIP kernels with a counter-based mask (csrc/fs2_dropout.hpp, include/dsf.h).

The mask of a dropout call is a pure function of (seed, step, site, element): for the flat index i of a float32 buffer

    q = i >> 2, j = i & 3
    w = Philox4x32-10(counter = (q lo32, q hi32, site, step lo32), key = (seed lo32, seed hi32))[j]
    element i is kept iff w >= thr,     thr = min(round(p * 2**32), 2**32 - 1),     kept elements are scaled by float32(1 / (1 - p))

- the generator of the sampler's noise (oracle/philox_oracle.py restates it in numpy).  Three things follow: the backward regenerates the mask
instead of reading a saved one (no tensor of the activation's size is kept per dropout site), a test computes the exact mask on the CPU, and
a FastSpeech2 training step is reproducible from (seed, step) alone.

OFF by default: while no state is enabled, FastSpeech2 in train mode draws from torch's generator through F.dropout exactly as before.

    from diffsinger_amd import dropout
    state = dropout.enable(seed=1234)          # EncSALayer, the embedding dropouts and the predictor stacks now use the HIP ops
    for batch in loader:
        loss = step(batch); loss.backward(); optimiser.step()
        state.advance()                        # AFTER backward(): the backward regenerates the masks of the step it belongs to

`site` numbers the dropout calls of one step in execution order (DropoutState.next_site); seed and step live in a device cell the kernels read,
so a captured training step stays valid when advance() - a device-side add - moves the step on."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib

_U32 = 0xFFFFFFFF


def mask_threshold(p: float) -> int:
    """thr of the contract: an element is kept iff its Philox word >= thr.  p in the open interval (0, 1)."""
    p = float(p)
    if not (0.0 < p < 1.0):
        raise ValueError(f'dropout probability must lie in the open interval (0, 1) (got {p!r}); bypass the op at p == 0')
    thr = min(int(round(p * 2 ** 32)), 2 ** 32 - 1)
    if thr == 0:
        raise ValueError(f'dropout probability {p!r} is below the resolution of the 32-bit mask (2**-33)')
    return thr


def mask_scale(p: float) -> float:
    """float32(1 / (1 - p)), the quotient formed in double (returned as a Python float that float32 holds exactly)."""
    mask_threshold(p)
    return float(np.float32(1.0 / (1.0 - float(p))))


class DropoutState:
    """The device cell {seed, step} the dropout kernels read, a host mirror of the step, and the site counter of the current step."""

    def __init__(self, device, seed: int):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('DropoutState: the dropout kernels have no CPU path - give a HIP device')
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.step = 0
        self._site = 0
        signed = self.seed - (1 << 64) if self.seed >> 63 else self.seed          # the cell holds the 64 bits; torch has no uint64 arithmetic
        self.cell = torch.tensor([signed, 0], dtype=torch.int64, device=self.device)

    def next_site(self) -> int:
        """The number of this dropout call inside the step (execution order)."""
        s = self._site
        self._site += 1
        return s

    def advance(self):
        """Next training step: step += 1 on the device in stream order (capturable), the site counter restarts.  Call it after backward()."""
        self.cell[1:].add_(1)
        self.step += 1
        self._site = 0


_STATE: Optional[DropoutState] = None


def enable(seed: int, device=None) -> DropoutState:
    """Switch FastSpeech2's train-mode dropouts to the HIP ops, from step 0 of `seed`.  device: default the current HIP device."""
    global _STATE
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    _STATE = DropoutState(device, seed)
    return _STATE


def disable():
    """Back to the default: train mode draws through F.dropout."""
    global _STATE
    _STATE = None


def current() -> Optional[DropoutState]:
    return _STATE


def _check(x: torch.Tensor, state: DropoutState, what: str):
    if not x.is_cuda:
        raise RuntimeError(f'{what}: the dropout kernels have no CPU path - move the tensors to the MI355X')
    if x.dtype != torch.float32:
        raise TypeError(f'{what}: float32 tensors only (got {x.dtype})')
    if x.device != state.device:
        raise RuntimeError(f'{what}: tensor on {x.device}, dropout state on {state.device}')


def _guard(ctx, what: str):
    if ctx.state.step != ctx.step:
        raise RuntimeError(f'{what}: the dropout state advanced from step {ctx.step} to {ctx.state.step} between forward and backward - the backward would '
                           f'regenerate another mask.  Call advance() after backward()')


def _dropout_raw(x, state, site, thr, scale):
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    if x.numel():
        _lib.call('dsf_dropout', x.device, x.data_ptr(), y.data_ptr(), x.numel(), state.cell.data_ptr(), site, thr, scale)
    return y


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, state, site, thr, scale):
        ctx.state, ctx.step, ctx.site, ctx.thr, ctx.scale = state, state.step, site, thr, scale
        return _dropout_raw(x, state, site, thr, scale)

    @staticmethod
    def backward(ctx, dy):
        _guard(ctx, 'dropout_op')
        return _dropout_raw(dy.contiguous(), ctx.state, ctx.site, ctx.thr, ctx.scale), None, None, None, None


def dropout_op(x: torch.Tensor, p: float, state: DropoutState, site: Optional[int] = None) -> torch.Tensor:
    """F.dropout(x, p, training=True) with the counter-based mask of (state, site) over x's flat (contiguous) indices; site=None takes the
    state's next site.  Saves nothing for the backward: the op is its own adjoint."""
    thr, scale = mask_threshold(p), mask_scale(p)
    _check(x, state, 'dropout_op')
    site = state.next_site() if site is None else int(site)
    return _Dropout.apply(x.contiguous(), state, site & _U32, thr, scale)


class _DropoutAddKeep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, keep, T, state, site, thr, scale):
        B, C, TS = x.shape
        ctx.state, ctx.step, ctx.site, ctx.thr, ctx.scale, ctx.keep, ctx.T = state, state.step, site, thr, scale, keep, T
        y = torch.empty_like(x)
        _lib.call('dsf_dropout_add_keep', x.device, x.data_ptr(), residual.data_ptr(), _lib.ptr(keep), y.data_ptr(), B, C, T, state.cell.data_ptr(),
                  site, thr, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        _guard(ctx, 'dropout_add_keep_op')
        dy = dy.contiguous()
        B, C, TS = dy.shape
        dx = torch.empty_like(dy)
        dres = torch.empty_like(dy) if ctx.needs_input_grad[1] else None
        _lib.call('dsf_dropout_add_keep_bwd', dy.device, dy.data_ptr(), _lib.ptr(ctx.keep), dx.data_ptr(), _lib.ptr(dres), B, C, ctx.T,
                  ctx.state.cell.data_ptr(), ctx.site, ctx.thr, ctx.scale)
        return dx if ctx.needs_input_grad[0] else None, dres, None, None, None, None, None, None


def dropout_add_keep_op(x: torch.Tensor, residual: torch.Tensor, keep: Optional[torch.Tensor], T: int, p: float, state: DropoutState,
                        site: Optional[int] = None) -> torch.Tensor:
    """(residual + F.dropout(x, p, True)) * keep on channel-major [B][C][TS] tensors (TS = padded_frames(T)) as ONE launch, zero in [T, TS);
    keep: float [B][T] of 0 / 1 or None.  The residual epilogue of an EncSALayer sub-block in train mode.  Saves no activation-sized tensor."""
    thr, scale = mask_threshold(p), mask_scale(p)
    _check(x, state, 'dropout_add_keep_op')
    _check(residual, state, 'dropout_add_keep_op')
    T = int(T)
    if x.dim() != 3 or residual.shape != x.shape or T < 1 or x.shape[2] != (T + 31) // 32 * 32:
        raise ValueError(f'dropout_add_keep_op: x and residual must be [B][C][padded_frames(T)] (got {tuple(x.shape)}, {tuple(residual.shape)}, T={T})')
    if keep is not None:
        if keep.shape != (x.shape[0], T) or keep.dtype != torch.float32 or keep.device != x.device:
            raise ValueError(f'dropout_add_keep_op: keep must be float32 [B][T] on the tensors\' device (got {tuple(keep.shape)}, {keep.dtype})')
        keep = keep.detach().contiguous()
    site = state.next_site() if site is None else int(site)
    return _DropoutAddKeep.apply(x.contiguous(), residual.contiguous(), keep, T, state, site & _U32, thr, scale)
