#!/usr/bin/env python3
"""Interleaved timing of float speaker verification (dsp_speaker_verif*) against the one existing per-(row, model)
yardstick, the enroller's statistics pass (dsp_speaker_enroll*), on the same rows:

    k 32, d 13 (the reference UBM), clips of 1 500 rows, S in {1, 64, 1024} speakers

    python tools/time_verify.py [--rows 1500] [--pairs 4e9] [--speakers 1 64 1024] [--rounds 7] [--calls 3] [--only verify_S64|enroll] [--clock-seconds 2]

For each S the clip count is chosen so that a call scores about --pairs (row, model) pairs (models = S + 1: the UBM is scored too), at
most 4 096 clips.  Within each round the enroller runs on the same rows between the verifier's calls (interleaved); `calls` launches go
out back to back with one synchronisation behind the last, and the per-launch time is the median and the minimum over the rounds, host
work included.  Printed per workload, one JSON line: (row, model) pairs per second for the verifier, rows per second for the enroller
(one model per row: its rows per second are its pairs per second).  The scorer does strictly less per pair than enroll_stats_kernel --
no F accumulation, no cross-lane reduction per row -- so a verifier slower per pair than the enroller means the layout has failed.
The box's clock: each workload is then run back to back for --clock-seconds while tools/gpu_sensors.py is read beside every group of
launches; the medians over the second half of that run are the `clock_under_load` line.
--only runs nothing but that workload's launches: the process to put under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_enroll import _clock_under_load, _time, _ubm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--pairs", type=float, default=4e9)
    ap.add_argument("--speakers", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_verify.py measures on a GPU: none found")
    ubm = _ubm()
    k, d = ubm["means"].shape
    gen = torch.Generator(device="cuda").manual_seed(7)
    max_clips = 4096
    feats = torch.randn((max_clips * args.rows, d), device="cuda", generator=gen)                  # rows shaped like CMVN'd features
    en = dsp_amd.SpeakerEnroller(ubm)
    ver = dsp_amd.SpeakerVerifier(ubm)
    mu = torch.tensor(np.asarray(ubm["means"], np.float32), device="cuda")
    work, shape = {}, {}
    for n_spk in args.speakers:
        clips = int(min(max_clips, max(1, round(args.pairs / ((n_spk + 1) * args.rows)))))
        fo = np.arange(clips + 1, dtype=np.int64) * args.rows
        means = (mu[None] + 0.05 * torch.randn((n_spk, k, d), device="cuda", generator=gen)).contiguous()
        x = feats[:clips * args.rows]
        work[f"verify_S{n_spk}"] = (lambda x=x, fo=fo, means=means: ver.verify(x, fo, means, want=("llr", "ll_ubm", "best", "best_llr")))
        shape[f"verify_S{n_spk}"] = {"clips": clips, "speakers": n_spk, "pairs": clips * args.rows * (n_spk + 1)}
    fo_all = np.arange(max_clips + 1, dtype=np.int64) * args.rows
    work["enroll"] = lambda: en.enroll(feats, fo_all)
    shape["enroll"] = {"clips": max_clips, "speakers": 0, "pairs": max_clips * args.rows}
    names = [args.only] if args.only else list(work)
    for name in names:                                   # warm-up: code objects, the span rings, the workspaces
        for _ in range(2):
            work[name]()
    if args.only:
        print(json.dumps({"workload": args.only, "ms": round(_time(torch, work[args.only], args.rounds * args.calls), 4)}), flush=True)
        return
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            if name != "enroll":
                res[name].append(_time(torch, work[name], args.calls))
                res["enroll"].append(_time(torch, work["enroll"], args.calls))       # the yardstick between every two of the verifier's
    for name in names:
        med, low = float(np.median(res[name])), float(min(res[name]))
        print(json.dumps(dict({"workload": name, "rows_per_clip": args.rows, "k": int(k), "d": int(d)}, **shape[name],
                              **{"ms_per_launch_median": round(med, 4), "ms_per_launch_min": round(low, 4),
                                 "pairs_per_s": round(shape[name]["pairs"] / (med * 1e-3), 0)})), flush=True)
    if args.clock_seconds > 0:
        from tools.gpu_sensors import Sensors
        sens = Sensors.for_device(0)
        print(json.dumps({"idle": sens.read()}), flush=True)
        for name in names:
            print(json.dumps(dict({"clock_under_load": name}, **_clock_under_load(torch, sens, work[name], args.clock_seconds))), flush=True)


if __name__ == "__main__":
    main()
