"""CPU: no contraction of the persistent Winograd loop copies its accumulators.

With -amdgpu-mfma-vgpr-form=1 an MFMA's destination is not tied to its C operand; across the back edge of a K loop (GemmPipe::run) hipcc then
let the chain end in other registers than it began in and moved the whole accumulator set back every iteration - 32 v_mov_b64 per six
chunks of the out-projection, eight in a row between two of its MFMAs, each a vector-ALU instruction paid in matrix time beside fp32 MFMAs.
The pipes of k_loop_wino_sa walk their chunks unrolled (GemmPipe::run_static / run_bounded): nothing is carried, nothing is copied.

What is counted: v_mov_b32 / v_mov_b64 between two CONSECUTIVE v_mfma_* of the listing - fewer than 8 wherever the two belong to one
contraction.  Two MFMAs with a barrier or a branch between them are not one contraction: what lies there is an epilogue and the next
prologue (the gate, the residual, the halo poll, the sampler update with its Philox constants - hundreds of instructions whose moves are
not copies of an accumulator set), and the listing of tools/isa_hashes.py carries no labels to tell a back edge from them otherwise.  The
copies this test is about sat in straight-line code between the last MFMAs of a loop body.  (A copy run that a compiler placed behind the
LAST MFMA of a looped body, in front of its back-edge branch, would escape this count; the pipes checked here have no loop left.)

The second test is the ISA pin of k_loop_wino_sa, by the rule of tests/test_verified_isa.py: the device code that ran on the MI355X
(its entries of tests/golden/kernel_isa_hashes.json) is what the sources still compile to, and every instantiation is listed."""
import json
import re

import pytest

from tests.test_verified_isa import _tool

# k_loop_wino_sa<HEAD_DDPM, 4>, <HEAD_PLMS, 4>: what the persistent path launches
KERNELS = ('k_loop_wino_saILi1ELi4EE', 'k_loop_wino_saILi2ELi4EE')
_SPLIT = re.compile(r'^(s_barrier|s_cbranch_\w+|s_branch|s_endpgm|s_setpc_b64)\b')


def _gaps(lines):
    """[(index of the first MFMA, moves between it and the next one, same contraction?)] for every pair of consecutive MFMAs"""
    out, last, moves, split = [], None, 0, False
    for i, ln in enumerate(lines):
        if ln.startswith('v_mfma_'):
            if last is not None:
                out.append((last, moves, not split))
            last, moves, split = i, 0, False
        elif ln.startswith('v_mov_b64') or ln.startswith('v_mov_b32'):
            moves += 1
        elif _SPLIT.match(ln):
            split = True
    return out


@pytest.mark.parametrize('kernel', KERNELS)
def test_no_register_copy_run_between_two_mfmas_of_a_contraction(kernel):
    listing = _tool().kernel_listing()
    names = [k for k in listing if kernel in k]
    assert len(names) == 1, names
    gaps = _gaps(listing[names[0]])
    inside = [g for g in gaps if g[2]]
    assert len(inside) >= 1000, 'the contractions of a layer and of the head are straight-line MFMA code'
    worst = max(inside, key=lambda g: g[1])
    print(f'{names[0]}: {len(gaps) + 1} MFMAs, {len(inside)} gaps inside a contraction, at most {worst[1]} v_mov in one of them')
    bad = [(i, n) for i, n, _ in inside if n >= 8]
    assert not bad, f'register-copy runs between two MFMAs of one contraction (instruction index, moves): {bad[:8]}'


def test_device_code_of_the_launched_winograd_loop_is_what_ran_on_the_gpu():
    mod = _tool()
    want = {k: v for k, v in json.load(open(mod.GOLDEN))['kernels'].items() if 'k_loop_wino_sa' in k}
    got = mod.kernel_hashes()
    assert sorted(want) == sorted(k for k in got if 'k_loop_wino_sa' in k), 'every instantiation of k_loop_wino_sa is listed'
    changed = [k for k in want if got[k] != want[k]]
    assert not changed, f'device code of k_loop_wino_sa changed without a GPU run (then: python tools/isa_hashes.py --update): {changed}'
