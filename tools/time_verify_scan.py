#!/usr/bin/env python3
"""Interleaved timing of the float speaker scan (dsp_speaker_float_scan_device) against the only other route to the same
numbers: a device gather of the cut-out windows into a ragged matrix of their own, then dsp_speaker_verify_ragged_device on it.

    k 32, d 13 (the reference UBM), recordings of 30 000 rows, window 98, hop 10, S in {1, 64, 1024} speakers

    python tools/time_verify_scan.py [--rows 30000] [--window 98] [--hop 10] [--pairs 1e9] [--speakers 1 64 1024] [--rounds 7] [--calls 3]
                                     [--only scan_S64|cut_S64] [--clock-seconds 2]

For each S the number of recordings is chosen so that the cut-out route scores about --pairs (row, model) pairs (models = S + 1), at most
64 recordings.  Within each round the two routes alternate (interleaved); `calls` launches go out back to back with one synchronisation
behind the last, and the per-launch time is the median and the minimum over the rounds, host work included.  The gather's index tensor is
built once, outside the timing; the gather itself (rows x 9.8 at 98 / 10) is inside, as a caller without the scan has to do it.  Both
routes are checked once to give the same bits.  Printed per S, one JSON line: both times, their ratio and window / hop, the bound the
arithmetic sets.  The box's clock: each workload is then run back to back for --clock-seconds while tools/gpu_sensors.py is read beside
every group of launches; the medians over the second half of that run are the `clock_under_load` line.
--only runs nothing but that workload's launches: the process to put under rocprofv3 --kernel-trace --stats for the split of the scan's
time between its two kernels."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_enroll import _clock_under_load, _time, _ubm  # noqa: E402

WANT = ("llr", "ll_ubm", "best", "best_llr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--window", type=int, default=98)
    ap.add_argument("--hop", type=int, default=10)
    ap.add_argument("--pairs", type=float, default=1e9)
    ap.add_argument("--speakers", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_verify_scan.py measures on a GPU: none found")
    ubm = _ubm()
    k, d = ubm["means"].shape
    gen = torch.Generator(device="cuda").manual_seed(7)
    max_rec = 64
    feats = torch.randn((max_rec * args.rows, d), device="cuda", generator=gen)                    # rows shaped like CMVN'd features
    ver = dsp_amd.SpeakerVerifier(ubm)
    mu = torch.tensor(np.asarray(ubm["means"], np.float32), device="cuda")
    per_rec = int(dsp_amd.scan_window_offsets([0, args.rows], args.window, args.hop)[-1])          # windows of one recording
    n_win = min(args.window, args.rows)
    work, shape = {}, {}
    for n_spk in args.speakers:
        rec = int(min(max_rec, max(1, round(args.pairs / ((n_spk + 1) * per_rec * n_win)))))
        fo = np.arange(rec + 1, dtype=np.int64) * args.rows
        x = feats[:rec * args.rows]
        means = (mu[None] + 0.05 * torch.randn((n_spk, k, d), device="cuda", generator=gen)).contiguous()
        start = (fo[:-1, None] + args.hop * np.arange(per_rec)[None]).reshape(-1)
        idx = torch.tensor((start[:, None] + np.arange(n_win)[None]).reshape(-1), device="cuda")
        clip_fo = np.arange(start.size + 1, dtype=np.int64) * n_win
        scan = (lambda x=x, fo=fo, means=means: ver.scan(x, fo, means, args.window, args.hop, want=WANT))
        cut = (lambda x=x, idx=idx, clip_fo=clip_fo, means=means: ver.verify(x[idx], clip_fo, means, want=WANT))
        a, b = scan(), cut()
        if not all(torch.equal(a[key], b[key]) for key in WANT):
            raise SystemExit(f"S {n_spk}: the scan and the cut-out route differ")
        work[f"scan_S{n_spk}"], work[f"cut_S{n_spk}"] = scan, cut
        shape[n_spk] = {"recordings": rec, "windows": int(start.size), "scan_pairs": rec * args.rows * (n_spk + 1),
                        "cut_pairs": int(start.size) * n_win * (n_spk + 1)}
    names = [args.only] if args.only else list(work)
    for name in names:                                   # warm-up: code objects, the span rings, the workspace
        for _ in range(2):
            work[name]()
    if args.only:
        print(json.dumps({"workload": args.only, "ms": round(_time(torch, work[args.only], args.rounds * args.calls), 4)}), flush=True)
        return
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:                               # scan_S, cut_S, scan_S', cut_S', ...: the two routes alternate
            res[name].append(_time(torch, work[name], args.calls))
    for n_spk in args.speakers:
        s, c = res[f"scan_S{n_spk}"], res[f"cut_S{n_spk}"]
        print(json.dumps(dict({"speakers": n_spk, "rows_per_recording": args.rows, "window": args.window, "hop": args.hop, "k": int(k), "d": int(d)},
                              **shape[n_spk], **{"scan_ms_median": round(float(np.median(s)), 4), "scan_ms_min": round(min(s), 4),
                                                 "cut_ms_median": round(float(np.median(c)), 4), "cut_ms_min": round(min(c), 4),
                                                 "cut_over_scan": round(float(np.median(c)) / float(np.median(s)), 3),
                                                 "window_over_hop": round(n_win / args.hop, 3),
                                                 "scan_pairs_per_s": round(shape[n_spk]["scan_pairs"] / (float(np.median(s)) * 1e-3), 0)})), flush=True)
    if args.clock_seconds > 0:
        from tools.gpu_sensors import Sensors
        sens = Sensors.for_device(0)
        print(json.dumps({"idle": sens.read()}), flush=True)
        for name in names:
            print(json.dumps(dict({"clock_under_load": name}, **_clock_under_load(torch, sens, work[name], args.clock_seconds))), flush=True)


if __name__ == "__main__":
    main()
