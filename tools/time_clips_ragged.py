#!/usr/bin/env python3
"""Ragged MFCC matrices against uniform clips, interleaved in one process (tools/time_clips.py's workload beside its ragged twin):

    uniform  12 500 x 1 s clips (BASELINE config 4's per-GPU share) through MfccPlan.clips
    ragged   the same total samples as seeded clips of 0.5 - 1.5 s (bench.py config5_ragged's lengths) through MfccPlan.clips_ragged

Prints one JSON line: median ms per call, its spread over the rounds, frames/s of each (the two frame counts differ slightly) and the
ragged / uniform frames/s ratio.

    python tools/time_clips_ragged.py [--clips 12500] [--rounds 9] [--calls 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dsp_amd  # noqa: E402
from dsp_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=12500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    n = args.clips
    gen = torch.Generator(device="cuda").manual_seed(1)
    clips = torch.rand((n, 16000), device="cuda", generator=gen) * 2 - 1
    # bench.py config5_ragged's recipe: 0.5 - 1.5 s, the last clip evening out the total
    rng = np.random.default_rng(1234)
    lens = rng.integers(8000, 24001, n)
    lens[-1] += 16000 * n - int(lens.sum()) if abs(16000 * n - int(lens.sum())) < 8000 else 0
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    flat = torch.rand(int(off[-1]), device="cuda", generator=gen) * 2 - 1
    c_off = L.c_offsets(off)

    plan = dsp_amd.MfccPlan()
    t_uni = dsp_amd.frames_for(plan.cfg, 16000, 500)
    f_uni = n * t_uni
    fo = dsp_amd.mfcc.ragged_frame_offsets(plan.cfg, c_off, 500)
    f_rag = int(fo[-1])
    out_u = torch.empty((n, t_uni, plan.cfg.n_mfcc), device="cuda")
    out_r = torch.empty((f_rag, plan.cfg.n_mfcc), device="cuda")
    uniform = lambda: plan.clips(clips, 500, out_u)                  # noqa: E731
    ragged = lambda: plan.clips_ragged(flat, c_off, 500, out=out_r)  # noqa: E731
    for _ in range(5):
        uniform()
        ragged()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    ts = {"uniform": [], "ragged": []}
    for r in range(args.rounds):                   # interleaved, the order alternating per round
        order = ("uniform", "ragged") if r % 2 == 0 else ("ragged", "uniform")
        for name in order:
            ts[name].append(timed(uniform if name == "uniform" else ragged))
    res = {"clips": n, "samples_uniform": 16000 * n, "samples_ragged": int(off[-1]), "frames_uniform": f_uni, "frames_ragged": f_rag,
           "rounds": args.rounds, "calls_per_round": args.calls}
    for name, frames in (("uniform", f_uni), ("ragged", f_rag)):
        v = np.array(ts[name])
        med = float(np.median(v))
        res[f"{name}_ms"] = round(med, 4)
        res[f"{name}_ms_min_max"] = [round(float(v.min()), 4), round(float(v.max()), 4)]
        res[f"{name}_frames_per_s"] = round(frames / (med * 1e-3), 0)
    res["ragged_over_uniform_frames_per_s"] = round(res["ragged_frames_per_s"] / res["uniform_frames_per_s"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
