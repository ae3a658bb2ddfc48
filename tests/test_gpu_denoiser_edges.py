"""GPU: the denoiser's 3-tap dilated convolution at short lengths on EVERY kernel that evaluates it, against the float64 oracle, with a bound the
reference sets (tests/denoiser_edge_helpers.py: 4 x the error of the float32 CPU form of the same sums, capped by the suite's flat figures).

Lengths (helpers.LENGTHS) put T <= d and T <= 2 d (an outer tap never meets the signal, a Winograd pair (t, t + d) straddles the end of the
utterance), the d frames on either side of a 32-frame tile boundary with and without a tile behind them, and an odd number of 32-frame tiles in
front of every kernel; B = 3 gives the middle utterance a neighbour on both sides of the tile list.  tests/test_denoiser_edges_host.py shows
that a tail that is not zeroed, a halo taken from the neighbouring utterance and a tap lost at a tile seam are 8000 x - 200000 x this bound at
every length where they can be seen.

  one layer      dsd_debug_layer: k_layer<1>, k_layer<2>, k_lat_conv<G> G = 2 / 4 / 8 / 16, k_lat_conv_w<G> G = 2 / 4 / 8 - dilations 1, 2, 4, 8
                 and the last layer
  one evaluation dsd_denoise with a step per utterance on the same nine settings
  K-step loops   k_loop (direct) and k_loop_wino_sa: DDPM K = 3 with explicit noise, PLMS 100 / 25
  chunk seam     T = 33 with one utterance more than a launch of the persistent loop holds: the utterances on both sides of the seam

Every comparison prints its measured maximum next to its bound and the share used (recorded: profiles/denoiser_edges_pytest_gpu.txt)."""
import pytest
import torch

from tests import denoiser_edge_helpers as E

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# (label, loop mode, layer tile, G, convolution): the nine settings of a single layer / a single evaluation
SETTINGS = ([('k_layer<1>', 0, 32, -1, 'direct'), ('k_layer<2>', 0, 64, -1, 'direct')]
            + [(f'k_lat_conv<{G}>', 3, 0, G, 'direct') for G in (2, 4, 8, 16)]
            + [(f'k_lat_conv_w<{G}>', 3, 0, G, 'winograd') for G in (2, 4, 8)])


@pytest.fixture(scope='module')
def gd():
    from tests.gpu_helpers import build_hip
    return build_hip(E.PRESET, 100)[0]


def _dev_cond(cond):
    """[B,H,T] view of a contiguous [B,T,H] device tensor - what the reference hands the denoiser"""
    return cond.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)


def _apply(eng, setting):
    """Select the kernels of `setting` and confirm with the getters that the prepared batch runs on them -> the yardstick's name."""
    label, mode, tile, G, conv = setting
    eng.set_loop_mode(mode)
    eng.set_layer_tile(tile)
    eng.set_lat_split(G)
    eng.set_conv_mode(conv)
    assert eng.loop_mode() == 0 and eng.loop_launches() == 0, label
    if mode == 0:
        assert (eng.lat_split(), eng.layer_tile(), eng.conv_mode()) == (0, tile, 0), label
    else:
        assert (eng.lat_split(), eng.layer_tile(), eng.conv_mode()) == (G, 32, 1 if conv == 'winograd' else 0), label
    return 'wino' if conv == 'winograd' else 'direct'


def _restore(eng):
    eng.set_loop_mode(2)
    eng.set_layer_tile(0)
    eng.set_lat_split(-1)
    eng.set_conv_mode('winograd')


@pytest.mark.parametrize('T', E.LENGTHS)
def test_one_layer_on_every_kernel(gd, T):
    inp, refs = E.inputs(T), E.layer_refs(T)
    eng = gd._engine(_dev_cond(inp['cond']))
    x = inp['x'].to(DEV)
    bad, base = [], {}
    try:
        for setting in SETTINGS:
            label, mode, tile, G, conv = setting
            yard = _apply(eng, setting)
            worst = None
            for l in E.LAYERS:
                xo, sk = eng.debug_layer(l, inp['t0'], x)
                last = l == E.LAYERS[-1]
                assert (xo is None) == last
                if label == 'k_layer<1>':
                    base[l] = (xo, sk)
                elif mode == 3 and conv == 'direct' and G < 8:              # the same k-ordered sums as k_layer
                    assert torch.equal(sk, base[l][1]) and (last or torch.equal(xo, base[l][0])), (label, l)
                for i, got in ((1, sk),) if last else ((0, xo), (1, sk)):
                    assert bool(torch.isfinite(got).all()), (label, l)
                    ref = refs[l]['ref'][i]
                    err, tol, ey = E.maxerr(got, ref), E.tolerance('layer', ref, refs[l][yard][i]), E.maxerr(refs[l][yard][i], ref)
                    row = (err / tol, err, tol, ey, l, ('x_out', 'skip')[i])
                    worst = row if worst is None or row > worst else worst
                    if err > tol:
                        bad.append((label,) + row)
            share, err, tol, ey, l, name = worst
            E.report(f'T={T} {label} worst of layers {E.LAYERS} at layer {l} {name}', err, tol, ey)
    finally:
        _restore(eng)
    assert not bad, bad


@pytest.mark.parametrize('T', E.SHORT)
def test_one_evaluation_on_every_path(gd, T):
    inp, refs = E.inputs(T), E.eval_refs(T)
    cond = _dev_cond(inp['cond'])
    eng = gd._engine(cond)
    spec, t = inp['spec'].to(DEV), inp['t'].to(DEV)
    bad = []
    try:
        for setting in SETTINGS:
            yard = _apply(eng, setting)
            with torch.no_grad():
                got = gd.denoise_fn(spec, t, cond)
            assert got.shape == refs['ref'].shape and bool(torch.isfinite(got).all()), setting[0]
            err, tol, ey = E.maxerr(got, refs['ref']), E.tolerance('eval', refs['ref'], refs[yard]), E.maxerr(refs[yard], refs['ref'])
            E.report(f'T={T} evaluation t={inp["t"].tolist()} {setting[0]}', err, tol, ey)
            if err > tol:
                bad.append((setting[0], err, tol))
    finally:
        _restore(eng)
    assert not bad, bad


def _loop(gd, kind, cond, x_T, noise):
    with torch.no_grad():
        if kind == 'ddpm':
            return gd.inference(cond, x_T=x_T, noise=noise, K_step=E.DDPM_K, pndm_speedup=0)
        return gd.inference(cond, x_T=x_T, K_step=E.PLMS_K, pndm_speedup=E.PLMS_INTERVAL)


@pytest.mark.parametrize('T', E.SHORT)
def test_k_step_loops_on_the_persistent_kernels(gd, T):
    inp = E.inputs(T, n_noise=E.DDPM_K)
    cond = _dev_cond(inp['cond'])
    eng = gd._engine(cond)
    x_T, noise = inp['spec'].to(DEV), inp['noise'].to(DEV)
    bad = []
    try:
        eng.set_loop_mode(1)
        for conv in ('winograd', 'direct'):
            eng.set_conv_mode(conv)
            for kind in ('ddpm', 'plms'):
                ref, yard = E.loop_refs(kind, T)
                got = _loop(gd, kind, cond, x_T, noise)
                assert eng.loop_mode() == 1 and eng.loop_launches() == 1 and eng.conv_mode() == (1 if conv == 'winograd' else 0)
                assert eng.loop_timeouts() == 0
                assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (conv, kind)
                err, tol = E.maxerr(got, ref), E.tolerance('mel' if kind == 'ddpm' else 'plms', ref, yard)
                E.report(f'T={T} {kind} loop, {conv} (max|mel| {float(ref.abs().max()):.2f})', err, tol, E.maxerr(yard, ref))
                if err > tol:
                    bad.append((conv, kind, err, tol))
    finally:
        _restore(eng)
    assert not bad, bad


def test_chunk_seam_of_the_persistent_loop(gd):
    """T = 33 (two tiles, one frame in the second) with B = one utterance more than a launch holds: the second launch runs a single utterance.
    Row 0, the last row of the first chunk and the row of the second chunk against the oracle, both convolution forms."""
    T = 33
    probe = gd._engine(torch.zeros(1, 256, T, device=DEV))
    try:
        probe.set_loop_mode(1)

        def launches(n):
            eng = gd._engine(torch.zeros(n, 256, T, device=DEV))
            assert eng is probe and eng.loop_mode() == 1
            return eng.loop_launches()
        assert launches(1) == 1
        hi = 2
        while launches(hi) < 2:                                     # B from the engine's own chunking, not from a CU count
            hi *= 2
            assert hi <= 4096, 'no second launch up to 4096 utterances'
        lo = hi // 2                                                # launches(lo) == 1 < launches(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if launches(mid) < 2 else (lo, mid)
        Bn, rows = hi, [0, hi - 2, hi - 1]
        inp = E.inputs(T, batch=Bn, n_noise=E.DDPM_K)
        cond = _dev_cond(inp['cond'])
        eng = gd._engine(cond)
        ref, yard = E.mel_refs('ddpm', inp['cond'][rows], inp['spec'][rows], inp['noise'][:, rows], k_step=E.DDPM_K)
        bad = []
        for conv in ('winograd', 'direct'):
            eng.set_conv_mode(conv)
            got = _loop(gd, 'ddpm', cond, inp['spec'].to(DEV), inp['noise'].to(DEV))
            assert eng.loop_mode() == 1 and eng.loop_launches() == 2 and eng.conv_mode() == (1 if conv == 'winograd' else 0)
            assert eng.loop_timeouts() == 0
            assert bool(torch.isfinite(got).all())
            for i, b in enumerate(rows):
                err, tol = E.maxerr(got[b], ref[i]), E.tolerance('mel', ref[i], yard[i])
                E.report(f'B={Bn} T={T} ddpm loop in 2 launches, {conv}, row {b}', err, tol, E.maxerr(yard[i], ref[i]))
                if err > tol:
                    bad.append((conv, b, err, tol))
    finally:
        _restore(probe)
    assert not bad, bad
