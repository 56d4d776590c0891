#!/usr/bin/env python3
"""Interleaved timing of UBM training (dsp_ubm_*) on the shape of the reference's train_ubm.py:

    2 500 000 rows x 13 coefficients (5 000 clips of about 500 CMVN'd rows), k = 32

    python tools/time_ubm.py [--rows 2500000] [--k 32] [--d 13] [--iters 20] [--rounds 5] [--fit-iters 300] [--only em|enroll|small]
                             [--no-cpu] [--clock-seconds 2]

Workloads, timed in turn within each round (interleaved):
    em       UbmTrainer.fit for --iters iterations at tol = 0 from a fixed start: ms per EM iteration and rows / s (the start's upload and
             the result's read-back are in it, once per fit)
    enroll   the same rows through SpeakerEnroller.enroll as one speaker: the E-step the library had before, over the same bytes -- what
             the second moments and the float64 tree cost is the difference
    small    6 000 rows, 300 iterations at tol = 0: a fit that is all launches; the time per iteration there is the price of a launch
             triple, which is what enqueueing without a host round trip buys (a synchronisation per iteration adds a round trip to each)
Then, once: the whole --fit-iters fit on the full rows, the clock and power under load (tools/gpu_sensors.py read beside the launches),
and the numpy restatement (tests/ubm_ref.py, float64) on 20 000 rows for one iteration on one core.  One JSON line per result.
--only runs nothing but that workload: the process to put under rocprofv3 --kernel-trace --stats or --pmc."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def _time(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _clock_under_load(torch, sens, fn, seconds):
    rows, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        mid = sens.read()
        e1.synchronize()
        rows.append((e0.elapsed_time(e1), mid.get("sclk_mhz"), mid.get("power_w")))
    late = rows[len(rows) // 2:]
    med = lambda i: float(np.median([r[i] for r in late if r[i] is not None])) if any(r[i] is not None for r in late) else None      # noqa: E731
    return {"calls": len(rows), "ms_per_call_gpu_median": round(med(0), 4), "sclk_mhz_median": med(1), "power_w_median": med(2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2500000)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--d", type=int, default=13)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fit-iters", type=int, default=300)
    ap.add_argument("--only", choices=["em", "enroll", "small"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    from tests import enroll_ref as E
    from tests import ubm_ref as U
    if not torch.cuda.is_available():
        raise SystemExit("time_ubm.py measures on a GPU: none found")
    k, d, n = args.k, args.d, args.rows
    rng = np.random.default_rng(1)
    truth = E.random_ubm(rng, k, d)
    var, w = 1.0 / truth["inv_covs"], E.weights_of(truth)
    gen = torch.Generator(device="cuda").manual_seed(7)
    comp = torch.multinomial(torch.from_numpy(w).cuda(), n, replacement=True, generator=gen)
    feats = (torch.from_numpy(truth["means"]).cuda()[comp] + torch.from_numpy(np.sqrt(var)).cuda()[comp]
             * torch.randn((n, d), device="cuda", dtype=torch.float64, generator=gen)).float().contiguous()
    del comp
    tr, small_tr = dsp_amd.UbmTrainer(k, d), dsp_amd.UbmTrainer(k, d)
    start = tr.init_rows(feats)
    en = dsp_amd.SpeakerEnroller({"log_consts": U.log_consts(start["weights"], start["variances"]), "means": start["means"], "inv_covs": 1.0 / start["variances"]})
    small = feats[:6000].contiguous()
    small_start = small_tr.init_rows(small)
    fo = np.array([0, n], np.int64)
    work = {"em": lambda: tr.fit(feats, init=start, max_iter=args.iters, tol=0.0),
            "enroll": lambda: en.enroll(feats, fo),
            "small": lambda: small_tr.fit(small, init=small_start, max_iter=300, tol=0.0)}
    per = {"em": args.iters, "enroll": 1, "small": 300}
    names = [args.only] if args.only else list(work)
    for name in names:                                   # warm-up: code objects, workspaces
        work[name]()
    if args.only:
        ms = float(np.median([_time(torch, work[args.only]) for _ in range(args.rounds)]))
        print(json.dumps({"workload": args.only, "ms_per_call": round(ms, 4), "ms_per_iteration": round(ms / per[args.only], 5)}), flush=True)
        return
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            res[name].append(_time(torch, work[name]) / per[name])
    for name in names:
        med, low = float(np.median(res[name])), float(min(res[name]))
        rows = 6000 if name == "small" else n
        floor = rows * d * 4 / HBM_BYTES_PER_S * 1e3
        print(json.dumps({"workload": name, "rows": rows, "k": k, "d": d, "iterations_per_call": per[name], "ms_per_iteration_median": round(med, 5),
                          "ms_per_iteration_min": round(low, 5), "rows_per_s": round(rows / (med * 1e-3), 0), "hbm_floor_ms": round(floor, 5),
                          "fraction_of_hbm_floor": round(floor / med, 4)}), flush=True)
    if args.fit_iters > 0:
        ms = _time(torch, lambda: tr.fit(feats, init=start, max_iter=args.fit_iters, tol=0.0))
        print(json.dumps({"workload": "whole_fit", "rows": n, "iterations": args.fit_iters, "seconds": round(ms * 1e-3, 4)}), flush=True)
    if args.clock_seconds > 0:
        from tools.gpu_sensors import Sensors
        sens = Sensors.for_device(0)
        print(json.dumps({"idle": sens.read()}), flush=True)
        for name in ("em", "enroll"):
            print(json.dumps(dict({"clock_under_load": name}, **_clock_under_load(torch, sens, work[name], args.clock_seconds))), flush=True)
    if not args.no_cpu:
        x = feats[:20000].cpu().numpy()
        t0 = time.perf_counter()
        U.fit(x, start, max_iter=1, tol=0.0)
        dt = time.perf_counter() - t0
        print(json.dumps({"workload": "cpu_numpy_restatement_one_core", "rows": 20000, "seconds_per_iteration": round(dt, 4), "rows_per_s": round(20000 / dt, 0)}), flush=True)


if __name__ == "__main__":
    main()
