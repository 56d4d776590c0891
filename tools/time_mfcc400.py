#!/usr/bin/env python3
"""The 400-point speaker front end beside the 512-point plan, on the same samples, alternating in one process:

    speaker  dsp_mfcc_speaker_config: n_fft 400, 128 mel filters, centred frames, DSP_LOG_GLOBAL_REF1 (mfcc400_kernel.hip)
    ref512   dsp_mfcc_default_config with DSP_LOG_GLOBAL_REF1: n_fft 512, 40 mel filters, complete frames -- the yardstick: the same
             two-pass log mode on the kernel every other number of this project is relative to

each over 12 500 equal clips of 1 s (BASELINE config 4's per-GPU share; MfccPlan.clips) and over a ragged batch of as many clips of
0.5 - 1.5 s (MfccPlan.clips_ragged).  Warmed up; prints one JSON line per workload (median and minimum ms per launch over the rounds,
frames per launch), the speaker / ref512 ratios, and the sensors idle and under each load.  No speed is promised: the 512-point plan
on the same machine in the same call is what the ratio is against.

    python tools/time_mfcc400.py [--clips 12500] [--rounds 9] [--calls 10] [--clock-seconds 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_enroll import _clock_under_load, _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=12500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    from dsp_amd import lib as L
    if not torch.cuda.is_available():
        raise SystemExit("time_mfcc400.py measures on a GPU: none found")
    n = args.clips
    gen = torch.Generator(device="cuda").manual_seed(1)
    clips = torch.rand((n, 16000), device="cuda", generator=gen) * 2 - 1
    rng = np.random.default_rng(1234)              # tools/time_clips_ragged.py's lengths
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(rng.integers(8000, 24001, n))
    flat = torch.rand(int(off[-1]), device="cuda", generator=gen) * 2 - 1
    c_off = L.c_offsets(off)
    plans = {"speaker": dsp_amd.MfccPlan(dsp_amd.speaker_config()),
             "ref512": dsp_amd.MfccPlan(dsp_amd.default_config(log_mode=L.LOG_GLOBAL_REF1))}
    cap = 2**31 - 1
    work, frames = {}, {}
    for name, plan in plans.items():
        t = dsp_amd.frames_for(plan.cfg, 16000, cap)
        fo = dsp_amd.ragged_frame_offsets(plan.cfg, c_off, cap)
        out_u = torch.empty((n, t, plan.cfg.n_mfcc), device="cuda")
        out_r = torch.empty((int(fo[-1]), plan.cfg.n_mfcc), device="cuda")
        work[f"{name}_equal"] = (lambda plan=plan, out=out_u: plan.clips(clips, cap, out))
        work[f"{name}_ragged"] = (lambda plan=plan, out=out_r: plan.clips_ragged(flat, c_off, cap, out=out))
        frames[f"{name}_equal"], frames[f"{name}_ragged"] = n * t, int(fo[-1])
    names = list(work)
    for _ in range(3):
        for name in names:
            work[name]()
    torch.cuda.synchronize()
    res = {name: [] for name in names}
    for r in range(args.rounds):                   # interleaved, the order alternating per round
        for name in (names if r % 2 == 0 else names[::-1]):
            res[name].append(_time(torch, work[name], args.calls))
    med = {}
    for name in names:
        med[name], low = float(np.median(res[name])), float(min(res[name]))
        print(json.dumps({"workload": name, "clips": n, "frames": frames[name], "ms_per_launch_median": round(med[name], 4),
                          "ms_per_launch_min": round(low, 4), "frames_per_s": round(frames[name] / (med[name] * 1e-3), 0)}), flush=True)
    print(json.dumps({"speaker_over_ref512_ms": {kind: round(med[f"speaker_{kind}"] / med[f"ref512_{kind}"], 3) for kind in ("equal", "ragged")},
                      "speaker_over_ref512_ms_per_frame": {kind: round(med[f"speaker_{kind}"] / frames[f"speaker_{kind}"]
                                                                 / (med[f"ref512_{kind}"] / frames[f"ref512_{kind}"]), 3)
                                                           for kind in ("equal", "ragged")}}), flush=True)
    if args.clock_seconds > 0:
        from tools.gpu_sensors import Sensors
        sens = Sensors.for_device(0)
        print(json.dumps({"idle": sens.read()}), flush=True)
        for name in names:
            print(json.dumps(dict({"clock_under_load": name}, **_clock_under_load(torch, sens, work[name], args.clock_seconds))), flush=True)


if __name__ == "__main__":
    main()
