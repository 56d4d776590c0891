#!/usr/bin/env python3
"""Interleaved timing of sliding CMVN and MAP enrolment (dsp_cmvn_*, dsp_speaker_enroll*) on the shape a fleet brings:

    4 096 speakers x 1 500 rows x 13 coefficients, one recording per speaker, CMVN window 300

    python tools/time_enroll.py [--speakers 4096] [--rows 1500] [--rounds 7] [--calls 3] [--only cmvn|enroll|both] [--no-cpu] [--clock-seconds 2]

Three workloads are timed in turn within each round (interleaved): CMVN alone, enrolment alone (on CMVN'd rows), and the two back to
back.  `calls` launches go out back to back with one synchronisation behind the last; the per-launch time is reported as the median
and the minimum over the rounds, host work included.  Floors are the algorithm's HBM bytes at 8 TB/s: CMVN reads and writes every row
once (2 x rows x d x 4 B), enrolment reads every row once (rows x d x 4 B; its chunk partials and outputs are not counted).  The CPU
baseline is the numpy restatement (tests/enroll_ref.py, float64) on 64 speakers, one core.  Prints one JSON line per workload.
The box's clock: each workload is then run back to back for --clock-seconds while tools/gpu_sensors.py is read beside every group of
launches (the readings are low-pass filtered over ~0.3 s, so a 3 ms launch alone shows the idle clock); the medians over the second half
of that run are the `clock_under_load` line.
--only runs nothing but that workload's launches: the process to put under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def _time(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def _clock_under_load(torch, sens, fn, seconds, group=8):
    """fn back to back for `seconds`, the sensors read while each group of launches runs -> medians over the second half"""
    rows, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(group):
            fn()
        e1.record()
        mid = sens.read()
        e1.synchronize()
        rows.append((e0.elapsed_time(e1) / group, mid.get("sclk_mhz"), mid.get("power_w")))
    late = rows[len(rows) // 2:]
    med = lambda i: float(np.median([r[i] for r in late if r[i] is not None])) if any(r[i] is not None for r in late) else None      # noqa: E731
    return {"groups": len(rows), "ms_per_launch_gpu_median": round(med(0), 4), "sclk_mhz_median": med(1), "power_w_median": med(2)}


def _ubm():
    """the reference UBM of the golden fixture where the tree has it, else a random one of its shape"""
    from tests import enroll_ref as E
    path = os.path.join(ROOT, "tests", "golden", "speaker_enroll_ref.npz")
    if os.path.exists(path):
        z = np.load(path)
        return {key: z[f"ubm_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
    return E.random_ubm(np.random.default_rng(1), 32, 13)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1500)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", choices=["cmvn", "enroll", "both"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    from tests import enroll_ref as E
    if not torch.cuda.is_available():
        raise SystemExit("time_enroll.py measures on a GPU: none found")
    ubm = _ubm()
    k, d = ubm["means"].shape
    n_rows = args.speakers * args.rows
    gen = torch.Generator(device="cuda").manual_seed(7)
    raw = torch.randn((n_rows, d), device="cuda", generator=gen) * 20.0            # rows shaped like compute_mfcc's
    raw[:, 0] = raw[:, 0] * 4.0 - 450.0
    fo = np.arange(args.speakers + 1, dtype=np.int64) * args.rows
    cm = dsp_amd.Cmvn(d, args.window)
    en = dsp_amd.SpeakerEnroller(ubm)
    feats = cm.apply(raw, fo)
    work = {"cmvn": lambda: cm.apply(raw, fo), "enroll": lambda: en.enroll(feats, fo), "both": lambda: en.enroll(cm.apply(raw, fo), fo)}
    floor = {"cmvn": 2 * n_rows * d * 4, "enroll": n_rows * d * 4, "both": 3 * n_rows * d * 4}
    names = [args.only] if args.only else list(work)
    for name in names:                                   # warm-up: code objects, the span rings, the enroller's workspace
        for _ in range(2):
            work[name]()
    if args.only:
        print(json.dumps({"workload": args.only, "ms": round(_time(torch, work[args.only], args.rounds * args.calls), 4)}), flush=True)
        return
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            res[name].append(_time(torch, work[name], args.calls))
    for name in names:
        med, low = float(np.median(res[name])), float(min(res[name]))
        print(json.dumps({"workload": name, "speakers": args.speakers, "rows_per_speaker": args.rows, "k": int(k), "d": int(d), "window": args.window,
                          "ms_per_launch_median": round(med, 4), "ms_per_launch_min": round(low, 4), "rows_per_s": round(n_rows / (med * 1e-3), 0),
                          "hbm_floor_bytes": floor[name], "hbm_floor_ms": round(floor[name] / HBM_BYTES_PER_S * 1e3, 4),
                          "fraction_of_hbm_floor": round(floor[name] / HBM_BYTES_PER_S * 1e3 / med, 4)}), flush=True)
    if args.clock_seconds > 0:
        from tools.gpu_sensors import Sensors
        sens = Sensors.for_device(0)
        print(json.dumps({"idle": sens.read()}), flush=True)
        for name in names:
            print(json.dumps(dict({"clock_under_load": name}, **_clock_under_load(torch, sens, work[name], args.clock_seconds))), flush=True)
    if not args.no_cpu:
        n_cpu = min(64, args.speakers)
        x = raw[:n_cpu * args.rows].cpu().numpy()
        t0 = time.perf_counter()
        y = E.cmvn_ragged(x, fo[:n_cpu + 1], args.window)
        t1 = time.perf_counter()
        E.enroll_ragged(y, fo[:n_cpu + 1], ubm)
        t2 = time.perf_counter()
        rows = n_cpu * args.rows
        print(json.dumps({"workload": "cpu_numpy_restatement_one_core", "speakers": n_cpu, "cmvn_rows_per_s": round(rows / (t1 - t0), 0),
                          "enroll_rows_per_s": round(rows / (t2 - t1), 0), "both_rows_per_s": round(rows / (t2 - t0), 0)}), flush=True)


if __name__ == "__main__":
    main()
