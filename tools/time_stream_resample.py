#!/usr/bin/env python3
"""Interleaved timing of the streaming resampler (dsp_stream_resample*) against the one-shot entry on the same samples:

    fw10     10 kHz float      -> 16 kHz, pushes of 1 000 frames (100 ms) per stream
    field48  48 kHz int16 mono -> 16 kHz, pushes of 4 800 frames (100 ms) per stream

    python tools/time_stream_resample.py [--shapes fw10 field48] [--streams 4096] [--rounds 7] [--calls 20] [--only SHAPE:SIDE]

Both sides get the same chunk buffer, `streams` chunks back to back.  `push` is StreamResampler.push (filter launch with the carried
history in front of every chunk, then the carry's copy launch); `oneshot` is Resampler.ragged, which treats every chunk as a recording
of its own (zeros in front: other outputs, the same work).  The sides are timed in turn within each round, `calls` calls back to back
with one synchronisation behind the last; per-call times are medians over the rounds, host work (planner, span tables) included.  The
first pushes are not timed: a stream's carry fills during them.  Bytes are the algorithm's: every chunk sample read once in its own
format, every output float written once, and for a push the carry read once and written once.  Prints one JSON line per shape.
--only SHAPE:SIDE (SIDE push | oneshot) runs nothing but that side: the process to put under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
SHAPES = {           # rate_in, dtype, frames per push (100 ms)
    "fw10": (10000, "float32", 1000),
    "field48": (48000, "int16", 4800),
}


def _make(torch, dsp_amd, name, streams):
    rate_in, dtype, frames = SHAPES[name]
    gen = torch.Generator(device="cuda").manual_seed(11)
    if dtype == "int16":
        x = torch.randint(-20000, 20000, (streams * frames,), device="cuda", generator=gen, dtype=torch.int16)
        sr = dsp_amd.StreamResampler(rate_in, 16000, streams, dtype=torch.int16)
    else:
        x = (torch.rand(streams * frames, device="cuda", generator=gen) * 2 - 1) * 0.5
        sr = dsp_amd.StreamResampler(rate_in, 16000, streams)
    one = dsp_amd.Resampler(rate_in, 16000)
    co = np.arange(streams + 1, dtype=np.int64) * frames
    offs = dsp_amd.lib.c_offsets(co)
    n_out = one.out_samples(frames)
    out = torch.empty((streams * (n_out + 1),), dtype=torch.float32, device="cuda")      # (a push emits n_out or one fewer or more)
    taps = (2 * one.half + one.up) // one.up
    es = x.element_size()
    info = {"shape": name, "rate_in": rate_in, "input": dtype, "streams": streams, "frames_per_push": frames, "up": one.up, "down": one.down,
            "taps_per_output": taps, "outputs_per_call": streams * n_out,
            "bytes_oneshot": streams * (frames * es + n_out * 4), "bytes_push": streams * (frames * es + n_out * 4 + 2 * (taps - 1) * es)}
    sides = {"push": lambda: sr.push(x, co, out=out), "oneshot": lambda: one.ragged(x, offs, out=out)}
    return sides, info, (sr, one, x, out)


def _time(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only")
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_stream_resample.py measures on a GPU: none found")
    if args.only:
        name, _, side = args.only.partition(":")
        if name not in SHAPES or side not in ("push", "oneshot"):
            raise SystemExit("--only takes SHAPE:push or SHAPE:oneshot")
        sides, _info, _keep = _make(torch, dsp_amd, name, args.streams)
        for _ in range(12):
            sides[side]()
        print(json.dumps({"shape": name, "side": side, "ms": round(_time(torch, sides[side], args.rounds * args.calls), 4)}), flush=True)
        return
    made = {name: _make(torch, dsp_amd, name, args.streams) for name in args.shapes}
    for name in args.shapes:                             # warm-up: code objects, the span rings' buffers, the streams' carries
        for _ in range(12):
            for fn in made[name][0].values():
                fn()
    res = {(name, side): [] for name in args.shapes for side in ("push", "oneshot")}
    for _ in range(args.rounds):
        for key in res:
            res[key].append(_time(torch, made[key[0]][0][key[1]], args.calls))
    for name in args.shapes:
        info = made[name][1]
        line = dict(info)
        for side in ("push", "oneshot"):
            ms = float(np.median(res[(name, side)]))
            rate = info["bytes_" + side] / (ms * 1e-3)
            line[side] = {"ms_per_call": round(ms, 4), "ms_range": [round(min(res[(name, side)]), 4), round(max(res[(name, side)]), 4)],
                          "bytes_per_s": round(rate, 0), "fraction_of_8TBps": round(rate / HBM_BYTES_PER_S, 4),
                          "gfma_per_s": round(info["outputs_per_call"] * info["taps_per_output"] / (ms * 1e-3) / 1e9, 1)}
        line["push_over_oneshot"] = round(line["push"]["ms_per_call"] / line["oneshot"]["ms_per_call"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
