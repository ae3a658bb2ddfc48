"""Host restatement of FastSpeech2's counter-based training dropout (diffsinger_amd/dropout.py, csrc/fs2_dropout.hpp): the mask from the
Philox oracle, and the three entry points of include/dsf.h in float32 numpy, every product and sum rounded once like the kernels' __fmul_rn /
__fadd_rn.  Written from the contract, not from the package: thr and scale are formed here again."""
import functools

import numpy as np

from oracle.philox_oracle import philox4x32_10

MASK32 = np.uint64(0xFFFFFFFF)


def thr_of(p: float) -> int:
    return min(int(round(p * 2 ** 32)), 2 ** 32 - 1)


def scale_of(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - p))


@functools.lru_cache(maxsize=8)
def words(seed: int, step: int, site: int, n: int) -> np.ndarray:
    """The Philox word of each of the flat indices 0..n-1: element i takes word i & 3 of quad i >> 2.  (Cached and read-only: a forward and its
    backward ask for the same mask.)"""
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    c = ((q & MASK32).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32), np.full(nq, site & 0xFFFFFFFF, dtype=np.uint32),
         np.full(nq, step & 0xFFFFFFFF, dtype=np.uint32))
    w = philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    out = np.stack(w, axis=1).reshape(-1)[:n]
    out.flags.writeable = False
    return out


def kept(seed: int, step: int, site: int, n: int, p: float) -> np.ndarray:
    """bool [n]: element i is kept iff its word >= thr (unsigned 32-bit compare)."""
    return words(seed, step, site, n) >= np.uint32(thr_of(p))


def dropout_ref(x: np.ndarray, seed: int, step: int, site: int, p: float) -> np.ndarray:
    """dsf_dropout on the flat float32 buffer x (any shape; C order)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    m = kept(seed, step, site, x.size, p).reshape(x.shape)
    return np.where(m, x * scale_of(p), np.float32(0)).astype(np.float32)


def _keep_full(keep, B, T, TS):
    k = np.ones((B, T), np.float32) if keep is None else np.asarray(keep, np.float32)
    return k[:, None, :]


def add_keep_ref(x, res, keep, T, seed, step, site, p):
    """dsf_dropout_add_keep on [B][C][TS] float32: keep * (res + (kept ? x * scale : 0)) in [0, T), exactly 0 in [T, TS)."""
    x, res = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(res, np.float32)
    B, C, TS = x.shape
    d = dropout_ref(x, seed, step, site, p)
    y = np.zeros_like(x)
    y[:, :, :T] = _keep_full(keep, B, T, TS) * (res[:, :, :T] + d[:, :, :T])
    return y


def add_keep_bwd_ref(dy, keep, T, seed, step, site, p):
    """dsf_dropout_add_keep_bwd: (dx, dres), dres = dy * keep, dx = kept ? dres * scale : 0, both 0 in [T, TS)."""
    dy = np.ascontiguousarray(dy, np.float32)
    B, C, TS = dy.shape
    dres = np.zeros_like(dy)
    dres[:, :, :T] = dy[:, :, :T] * _keep_full(keep, B, T, TS)
    return dropout_ref(dres, seed, step, site, p), dres
