"""Developer tool (GPU): one FastSpeech2 training step (forward + backward, TRAIN mode: dropout 0.1 in the FFT blocks, predictor_dropout 0.5)
at the bench shape (8 utterances x 128 phones x 8 frames = 1024 mel frames each) with the counter-based HIP dropout (diffsinger_amd/dropout.py)
switched off - torch's F.dropout, the default - and on, ALTERNATING in one process.  One JSON line: per mode the median / min / max over the
rounds of the mean step time, and the peak allocated memory of one step.      python tools/bench_fs2_dropout.py [rounds] [steps_per_round]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import diffsinger_amd
from diffsinger_amd import dropout, hparams


def main(rounds=7, steps=10, preset='lj_ds_beta6', B=8, T_txt=128, frames_per_phone=8):
    hparams.clear()
    diffsinger_amd.use_preset(preset)
    from diffsinger_amd import fs2
    dev = torch.device('cuda', 0)
    torch.manual_seed(1234)
    m = fs2.FastSpeech2(63, 80).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(7)
    tok = torch.randint(1, 63, (B, T_txt), device=dev, generator=g)
    T = T_txt * frames_per_phone
    mel2ph = (torch.arange(T, device=dev) // frames_per_phone + 1)[None].repeat(B, 1)
    f0 = torch.rand(B, T, device=dev, generator=g) * 2 + 6.5
    uv = torch.zeros(B, T, device=dev)

    def step():
        m.zero_grad(set_to_none=True)
        r = m(tok, mel2ph=mel2ph, f0=f0.clone(), uv=uv, infer=False)
        loss = r['mel_out'].abs().mean() + r['dur'].square().mean()
        if torch.is_tensor(r.get('pitch_pred')) and r['pitch_pred'].requires_grad:
            loss = loss + r['pitch_pred'].square().mean()
        loss.backward()
        st = dropout.current()
        if st is not None:
            st.advance()
        return loss

    def switch(on):
        if on:
            if dropout.current() is None:
                dropout.enable(1234, dev)
        else:
            dropout.disable()

    times, peak, loss = {False: [], True: []}, {}, {}
    for on in (False, True):                                            # warm-up of both paths: code objects, packed weights, the allocator
        switch(on)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        loss[on] = float(step().detach())
        torch.cuda.synchronize()
        peak[on] = torch.cuda.max_memory_allocated(dev)
    for _ in range(rounds):
        for on in (False, True):
            switch(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            times[on].append((time.perf_counter() - t0) / steps * 1e3)
    dropout.disable()
    out = {'preset': preset, 'B': B, 'T_mel': T, 'rounds': rounds, 'steps_per_round': steps, 'dropout': hparams['dropout'],
           'predictor_dropout': hparams['predictor_dropout']}
    for on, name in ((False, 'off'), (True, 'on')):
        out[name] = {'ms_median': statistics.median(times[on]), 'ms_min': min(times[on]), 'ms_max': max(times[on]),
                     'peak_allocated_MiB': peak[on] / 2 ** 20, 'loss': loss[on]}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:3]]
    main(*a)
