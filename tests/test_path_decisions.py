"""CPU: which kernels a prepared batch runs on is ONE pure function (csrc/dsd_path.hpp, sampler_path).  tests/path_table.cpp prints its
result for a fixed grid of inputs - CU counts, layer counts, batch shapes, every loop mode / lat_split / layer tile / convolution / split /
graph / parked setting - as canonical text.  tests/golden/path_decisions.json holds the sha256 of that table and rows of it spelled out;
it was recorded from lat_g, layer_nb, loop_applicable and wino_applicable as they stood in dsd.hip, moved into the header with nothing but
`h->` turned into `in.`, BEFORE they were collapsed into sampler_path: the decision did not change with the refactor."""
import functools
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('n_cu', 'L', 'B', 'T', 'loop', 'lat', 'tile', 'conv', 'split', 'graph', 'off')


@functools.lru_cache(maxsize=None)
def path_table_binary() -> str:
    """tests/path_table.cpp compiled for the host (once per session)."""
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    out = os.path.join(tempfile.mkdtemp(prefix='path_table_'), 'path_table')
    subprocess.run([cxx, '-std=c++17', '-O1', '-o', out, os.path.join(ROOT, 'tests', 'path_table.cpp')], check=True)
    return out


def decide(**kw) -> dict:
    """The decision for one input (keys: FIELDS) as {'kind': ..., 'G': ..., 'frames': ..., 'lat_wino': ..., 'upc': ..., 'launches': ..., 'key': ...}."""
    line = subprocess.run([path_table_binary()] + [str(int(kw[f])) for f in FIELDS], check=True, capture_output=True, text=True).stdout.strip()
    head, res = line.split(' -> ')
    assert head == ' '.join(f'{f}={int(kw[f])}' for f in FIELDS), line
    kind, *rest = res.split()
    return {'kind': kind, **{k: int(v) for k, v in (r.split('=') for r in rest)}}


def test_path_decisions_are_the_recorded_ones():
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'path_decisions.json')))
    txt = subprocess.run([path_table_binary()], check=True, capture_output=True).stdout
    lines = txt.decode().splitlines()
    assert len(lines) == gold['lines'] == 4 * 2 * 7 * 9 * 4 * 6 * 3 * 2 * 2 * 2 * 2
    have = set(lines)
    assert len(gold['rows']) >= 60
    wrong = [r for r in gold['rows'] if r not in have]
    assert not wrong, f'path decisions differ from the recorded rows: {wrong[:4]}'
    assert hashlib.sha256(txt).hexdigest() == gold['sha256'], 'the decision table changed somewhere outside the spelled-out rows'


def test_single_query_prints_the_row_of_the_table():
    got = decide(n_cu=256, L=20, B=8, T=1024, loop=2, lat=-1, tile=0, conv=1, split=0, graph=1, off=0)
    assert got == {'kind': 'persistent-winograd', 'G': 0, 'frames': 32, 'lat_wino': 0, 'upc': 8, 'launches': 1, 'key': 10001}
    got = decide(n_cu=256, L=20, B=5, T=1024, loop=2, lat=-1, tile=0, conv=0, split=0, graph=1, off=0)
    assert got['kind'] == 'latency' and got['G'] == 8 and got['lat_wino'] == 0
