"""CPU restatement of the free-running duration path for the length-regulator tests: DurationPredictor.out2dur followed by
LengthRegulator.forward (modules/fastspeech/tts_modules.py:122-131, :158-186), written from the contract in include/dsf.h
(dsf_length_regulate), not from the code under test: an inclusive running sum and an upper-bound search instead of the [B, T_txt, T_mel]
mask.  tests/test_length_regulate_host.py pins it to the recorded reference results."""
import torch


def out2dur64(logdur: torch.Tensor, offset: float = 1.0) -> torch.Tensor:
    """out2dur in float64: max(round_half_even(exp(y) - offset), 0) as int64."""
    return torch.clamp(torch.round(logdur.double().exp() - offset), min=0).long()


def half_distance64(logdur: torch.Tensor, offset: float = 1.0) -> torch.Tensor:
    """|frac(exp(y) - offset) - 0.5| in float64: how far a token is from the rounding boundary of out2dur."""
    v = logdur.double().exp() - offset
    return ((v - torch.floor(v)) - 0.5).abs()


def regulate(dur=None, logdur=None, padding=None, alpha=1.0, T_out=None, offset=1.0):
    """-> (dur_choice int64 [B,T_txt] or None in the integer form, mel2ph int64 [B,T_out], mel_len int64 [B], not clipped).
    T_out=None: the longest row (the reference's axis)."""
    assert (dur is None) != (logdur is None)
    choice = None
    if logdur is not None:
        choice = torch.clamp(torch.round(logdur.float().exp() - offset), min=0).long()        # fp32, one rounding per operation
        dur = choice
    d = torch.round(dur.float() * alpha).long()
    if padding is not None:
        d = torch.where(padding.bool(), torch.zeros_like(d), d)
    cum = torch.cumsum(d, 1)                                                                   # int64, inclusive
    mel_len = cum[:, -1].clone()
    if T_out is None:
        T_out = int(mel_len.max())
    t = torch.arange(T_out)[None].expand(d.shape[0], T_out).contiguous()
    j = torch.searchsorted(cum, t, right=True)                                                 # first token whose running sum exceeds t
    mel2ph = torch.where(t < mel_len[:, None], j + 1, torch.zeros_like(j))
    return choice, mel2ph, mel_len


def pad_frames(mel2ph: torch.Tensor, N: int) -> torch.Tensor:
    """mel2ph [B,T] -> [B,N]: padding frames (0) appended, or the rows cut at N."""
    B, T = mel2ph.shape
    out = torch.zeros(B, N, dtype=mel2ph.dtype, device=mel2ph.device)
    out[:, :min(T, N)] = mel2ph[:, :min(T, N)]
    return out
