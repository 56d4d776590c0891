#!/usr/bin/env python3
"""Interleaved timing of the polyphase FIR resampler (dsp_resample_*) on the shapes its users bring:

    field48  48 kHz int16 mono -> 16 kHz, 2 000 recordings of 30 s           (dsp_resample_ragged_pcm16_device)
    field44  44.1 kHz float    -> 16 kHz, 2 000 recordings of 30 s           (dsp_resample_ragged_device)
    fw10     10 kHz float      -> 16 kHz, 125 000 one-second clips           (dsp_resample_clips_device)

    python tools/time_resample.py [--shapes field48 field44 fw10] [--scale 1.0] [--rounds 7] [--calls 5] [--only SHAPE]

The shapes are timed in turn within each round (interleaved), `calls` launches back to back with one synchronisation behind the last;
the per-launch time is the median over the rounds, host work included.  Bytes are the algorithm's: every input sample read once in
its own format, every output float written once -- the filter history a tile re-reads is not counted.  Prints one JSON line per shape
with bytes/s against the 8 TB/s HBM roofline and the FMA rate (taps per output x outputs).  --scale shrinks the batch (a rehearsal);
--only SHAPE runs nothing but that shape's launches: the process to put under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
SHAPES = {           # rate_in, dtype, recordings, seconds, entry
    "field48": (48000, "int16", 2000, 30, "ragged"),
    "field44": (44100, "float32", 2000, 30, "ragged"),
    "fw10": (10000, "float32", 125000, 1, "clips"),
}


def _make(torch, dsp_amd, name, scale):
    rate_in, dtype, n_rec, seconds, entry = SHAPES[name]
    n_rec = max(1, int(n_rec * scale))
    n = rate_in * seconds
    rs = dsp_amd.Resampler(rate_in, 16000)
    gen = torch.Generator(device="cuda").manual_seed(7)
    if dtype == "int16":
        x = torch.randint(-20000, 20000, (n_rec * n,), device="cuda", generator=gen, dtype=torch.int16)
    else:
        x = (torch.rand(n_rec * n, device="cuda", generator=gen) * 2 - 1) * 0.5
    n_out = rs.out_samples(n)
    if entry == "clips":
        x = x.view(n_rec, n)
        out = torch.empty((n_rec, n_out), dtype=torch.float32, device="cuda")

        def run():
            return rs.clips(x, out=out)
    else:
        offs = dsp_amd.lib.c_offsets(np.arange(n_rec + 1, dtype=np.int64) * n)
        out = torch.empty((n_rec * n_out,), dtype=torch.float32, device="cuda")

        def run():
            return rs.ragged(x, offs, out=out)
    taps_per_output = (2 * rs.half + rs.up) // rs.up
    info = {"shape": name, "rate_in": rate_in, "input": dtype, "recordings": n_rec, "seconds": seconds, "entry": entry, "up": rs.up, "down": rs.down,
            "bytes": n_rec * (n * x.element_size() + n_out * 4), "outputs": n_rec * n_out, "taps_per_output": taps_per_output}
    return run, info, (rs, x, out)


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
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", choices=list(SHAPES))
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_resample.py measures on a GPU: none found")
    names = [args.only] if args.only else args.shapes
    made = {name: _make(torch, dsp_amd, name, args.scale) for name in names}
    for name in names:                                   # warm-up: code objects, the span ring's buffers
        for _ in range(3):
            made[name][0]()
    if args.only:
        print(json.dumps({"shape": args.only, "ms": round(_time(torch, made[args.only][0], args.rounds * args.calls), 4)}), flush=True)
        return
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            res[name].append(_time(torch, made[name][0], args.calls))
    for name in names:
        info = made[name][1]
        ms = float(np.median(res[name]))
        rate = info["bytes"] / (ms * 1e-3)
        print(json.dumps(dict(info, ms_per_launch=round(ms, 4), ms_range=[round(min(res[name]), 4), round(max(res[name]), 4)],
                              bytes_per_s=round(rate, 0), fraction_of_8TBps=round(rate / HBM_BYTES_PER_S, 4),
                              gfma_per_s=round(info["outputs"] * info["taps_per_output"] / (ms * 1e-3) / 1e9, 1))), flush=True)


if __name__ == "__main__":
    main()
