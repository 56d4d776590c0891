#!/usr/bin/env python3
"""Timing of stop-net training at the reference's shape: 13 x 500 inputs, units 4-2-2-1, clips of 98 frames (F_used
1 274), 2 000 training rows and 500 validation rows, batch 32 (63 steps an epoch), for 1, 16 and 256 runs per launch set.

    python tools/time_stoptrain.py [--runs 1 16 256] [--epochs 4] [--rounds 5] [--no-restatement]

A launch set is one StopTrainer.train call: the init launch, one launch per epoch with every run in it, the finish launch.  Times are
between HIP events on the call's stream, after one warm-up call, medians over the rounds.  `step_us` is the set's time over epochs x
steps, with every run sharing that time; `model_bytes_per_step` is what one step of one run moves by the design's count -- kernel1
read once by the forward pass, kernel1 and both Adam moments read and written by the update (7 x F_used x u1 x 8 bytes), the batch's Z
rows read by the forward pass and again by the gradient (2 x B x F_used x 4) -- and `achieved_gb_s` that count times the runs over
step_us.  The restatement's time for one run on one host core is printed beside them as a baseline, not a gate.  One JSON line per
run count."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_COEF, MAX_FRAMES, UNITS, FRAMES, N_TRAIN, N_VAL, BATCH = 13, 500, (4, 2, 2, 1), 98, 2000, 500, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    import torch
    from dsp_amd import consumers as dc
    if not torch.cuda.is_available():
        raise SystemExit("time_stoptrain.py measures on a GPU: none found")
    n = N_TRAIN + N_VAL
    rng = np.random.default_rng(0)
    labels = (np.arange(n) % 2).astype(np.int32)
    mfcc = (rng.standard_normal((n * FRAMES, N_COEF)) * 3.0 + labels.repeat(FRAMES)[:, None] * 0.5).astype(np.float32)
    fo = np.arange(n + 1, dtype=np.int64) * FRAMES
    train_rows, val_rows = np.arange(N_TRAIN, dtype=np.int32), np.arange(N_TRAIN, n, dtype=np.int32)
    t = dc.StopTrainer(N_COEF, MAX_FRAMES, UNITS)
    d_mfcc = torch.from_numpy(mfcc).cuda()
    t.set(d_mfcc, fo, scaler_rows=train_rows)
    steps = -(-N_TRAIN // BATCH)
    model_bytes = 7 * t.f_used * UNITS[0] * 8 + 2 * BATCH * t.f_used * 4
    for n_runs in args.runs:
        runs = [dict(train_rows=train_rows, val_rows=val_rows, seed=s, epochs=args.epochs, patience=args.epochs, batch_size=BATCH) for s in range(n_runs)]
        t.train(runs, labels, prob=False)                                     # warm-up: code objects, the ring, the workspace
        ms = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = t.train(runs, labels, prob=False)[0]
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        step_us = med * 1e3 / (args.epochs * steps)
        print(json.dumps({"runs": n_runs, "epochs": args.epochs, "steps_per_epoch": steps, "f_used": t.f_used, "set_ms_median": round(med, 3),
                          "set_ms_min": round(min(ms), 3), "epoch_ms": round(med / args.epochs, 3), "step_us": round(step_us, 2),
                          "step_us_per_run": round(step_us / n_runs, 3), "model_bytes_per_step": model_bytes,
                          "achieved_gb_s": round(model_bytes * n_runs / (step_us * 1e-6) / 1e9, 2), "dead_runs": int((res["n_dead_units"] > 0).sum())}), flush=True)
    if not args.no_restatement:
        from tests import stoptrain_ref as R
        z = t.rows()
        t0 = time.perf_counter()
        R.train_run(z, labels, N_COEF, MAX_FRAMES, UNITS, dict(train_rows=train_rows, val_rows=val_rows, seed=0, epochs=args.epochs, patience=args.epochs, batch_size=BATCH))
        print(json.dumps({"restatement_one_run_ms": round((time.perf_counter() - t0) * 1e3, 1), "epochs": args.epochs}), flush=True)
    t.close()


if __name__ == "__main__":
    main()
