"""A plain restatement of the four formulas of stream sessions (include/dsp_amd.h "LIVE STREAMS"), for the tests: rows and windows
that exist after N samples, what a push emits, what the session carries.  No library call in here."""
import numpy as np

CHUNKS = [0, 1, 159, 160, 161, 399, 400, 401, 1600, 16000, 50001]


def rows_after(n, fl, h):
    return 1 + (n - fl) // h if n >= fl else 0


def windows_after(e, wf, hf):
    return 1 + (e - wf) // hf if e >= wf else 0


def carried_samples(n, fl, h):
    return n - rows_after(n, fl, h) * h


def carried_rows(e, wf, hf):
    return e - windows_after(e, wf, hf) * hf


def push_plan(received, lengths, fl, h, wf=None, hf=None):
    """-> (row_offsets, window_offsets | None) of a push of `lengths[s]` samples to streams that hold `received[s]`"""
    ro, wo = [0], [0]
    for n0, ln in zip(received, lengths):
        e0, e1 = rows_after(n0, fl, h), rows_after(n0 + ln, fl, h)
        ro.append(ro[-1] + e1 - e0)
        if wf is not None:
            wo.append(wo[-1] + windows_after(e1, wf, hf) - windows_after(e0, wf, hf))
    return np.array(ro, np.int64), (np.array(wo, np.int64) if wf is not None else None)


def chunking(total, rng, choices=CHUNKS):
    """seeded chunk lengths that add up to `total` (the last one cut to fit)"""
    out, left = [], total
    while left > 0:
        c = min(int(rng.choice(choices)), left)
        out.append(c)
        left -= c
    return out
