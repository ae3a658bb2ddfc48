"""Developer tool (GPU): the FastSpeech2 forward as inference runs it - ONE utterance, FREE-RUNNING (mel2ph=None: the duration predictor
chooses the durations) - on the torch length regulator with its host read (the parent's path), on dsf_length_regulate, on a frame budget
(max_frames=N, no host read) and as a hipGraph replay of the budgeted forward; the teacher-forced forward at the same shape for orientation.

    python tools/bench_free.py [T_txt] [window_s] [repeats]  > profiles/<name>.jsonl

Synthetic weights give arbitrary durations, so the duration predictor's last layer is set (small weight, bias log(1 + 8)) to ~8 frames per
phone.  Per mode and call: host wall time of a window that ends in a synchronise, and device time between two events around the call (a
launch-bound forward's device time contains the gaps the host leaves).  The modes are interleaved inside every repeat, so drift between
processes or boxes does not enter; mean and spread (max - min) over the repeats."""
import datetime
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import diffsinger_amd
from diffsinger_amd import _lib, fs2, hparams
from diffsinger_amd.graphs import GraphedForward

PRESETS = ('lj_ds_beta6', 'opencpop_ds1000')


def setup(preset, T_txt, dev, frames_per_phone=8):
    hparams.clear()
    diffsinger_amd.use_preset(preset)
    torch.manual_seed(1234)
    midi = bool(hparams.get('use_midi'))
    m = (fs2.FastSpeech2MIDI if midi else fs2.FastSpeech2)(63, 80).eval()
    with torch.no_grad():
        m.dur_predictor.linear.weight.mul_(0.01)
        m.dur_predictor.linear.bias.fill_(math.log(1 + frames_per_phone))
    g = torch.Generator().manual_seed(7)
    tok = torch.randint(1, 63, (1, T_txt), generator=g)
    kw = {}
    if midi:
        kw = dict(pitch_midi=torch.randint(40, 80, (1, T_txt), generator=g), midi_dur=torch.rand(1, T_txt, generator=g),
                  is_slur=torch.randint(0, 2, (1, T_txt), generator=g))
    return m.to(dev), tok.to(dev), {k: v.to(dev) for k, v in kw.items()}


def wall_ms(f, window_s):
    """Host wall per call over a window of at least window_s that ends in a synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(10):
            f()
        n += 10
        if time.perf_counter() - t0 >= window_s:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, n


def device_ms(f, calls=100):
    """Mean time between an event recorded before and one recorded after each call (the stream is drained before every call)."""
    tot = 0.0
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        f()
        b.record()
        b.synchronize()
        tot += a.elapsed_time(b)
    return tot / calls


def stats(v):
    return {'mean': round(sum(v) / len(v), 4), 'spread': round(max(v) - min(v), 4), 'runs': [round(x, 4) for x in v]}


@torch.no_grad()
def run(preset, T_txt, window_s, repeats, dev):
    m, tok, kw = setup(preset, T_txt, dev)
    keys = sorted(kw)
    vals = [kw[k] for k in keys]
    first = m(tok, infer=True, **kw)
    mel_len = int(first['mel_len'].max())
    N = (mel_len // 64 + 1) * 64
    mel2ph = first['mel2ph'].clone()

    def parent():
        fs2.set_regulate_native(regulate=False)
        try:
            return m(tok, infer=True, **kw)
        finally:
            fs2.set_regulate_native(True, True)

    g_free = GraphedForward(lambda t, *v: m(t, infer=True, max_frames=N, **dict(zip(keys, v))))
    g_teacher = GraphedForward(lambda t, m2p, *v: m(t, mel2ph=m2p, infer=True, **dict(zip(keys, v))))
    modes = {
        'a_parent_torch_regulator_eager': parent,
        'b_operator_no_budget_eager': lambda: m(tok, infer=True, **kw),
        'c_operator_budget_eager': lambda: m(tok, infer=True, max_frames=N, **kw),
        'd_operator_budget_graph_replay': lambda: g_free(tok, *vals),
        'teacher_forced_eager': lambda: m(tok, mel2ph=mel2ph, infer=True, **kw),
        'teacher_forced_graph_replay': lambda: g_teacher(tok, mel2ph, *vals),
    }
    # the budgeted forward computes what the others compute (same integers on the real frames)
    assert torch.equal(modes['c_operator_budget_eager']()['mel2ph'][:, :mel_len], mel2ph) and torch.equal(parent()['mel2ph'], mel2ph)
    for f in modes.values():                                   # warm every shape (weight packing, graph capture, code objects)
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    wall = {k: [] for k in modes}
    devt = {k: [] for k in modes}
    calls = {}
    for _ in range(repeats):
        for k, f in modes.items():
            w, calls[k] = wall_ms(f, window_s)
            wall[k].append(w)
            devt[k].append(device_ms(f))
    row = {'tool': 'tools/bench_free.py', 'preset': preset, 'shape': f'1 utterance, {T_txt} phones, free-running', 'mel_len': mel_len, 'max_frames': N,
           'window_s': window_s, 'repeats': repeats, 'calls_in_last_window': calls, 'unit': 'ms per forward',
           'wall': {k: stats(v) for k, v in wall.items()}, 'device': {k: stats(v) for k, v in devt.items()}}
    a, b, d = row['wall']['a_parent_torch_regulator_eager'], row['wall']['b_operator_no_budget_eager'], row['wall']['d_operator_budget_graph_replay']
    noise = max(a['spread'], b['spread'], d['spread'])
    row['acceptance'] = {
        'spread_ms': noise,
        'b_not_slower_than_a': bool(b['mean'] <= a['mean'] + noise),
        'd_faster_than_a': bool(d['mean'] < a['mean'] - noise),
        'a_over_d_wall': round(a['mean'] / d['mean'], 3),
        'd_wall_over_device': round(d['mean'] / row['device']['d_operator_budget_graph_replay']['mean'], 3),
        'budget_price_device_c_over_b': round(row['device']['c_operator_budget_eager']['mean'] / row['device']['b_operator_no_budget_eager']['mean'], 3),
    }
    row['measured'] = {'device': torch.cuda.get_device_name(0), 'date': datetime.date.today().isoformat(), 'build_id': _lib.build_id()[:16]}
    return row


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    T_txt = int(args[0]) if len(args) > 0 else 100
    window_s = float(args[1]) if len(args) > 1 else 1.0
    repeats = int(args[2]) if len(args) > 2 else 3
    dev = torch.device('cuda', 0)
    for preset in PRESETS:
        print(json.dumps(run(preset, T_txt, window_s, repeats, dev)), flush=True)


if __name__ == '__main__':
    main()
