#!/usr/bin/env python3
"""Timing of dsp_calibration_fit_device and dsp_calibration_apply_device at three shapes:

    reference  92 x 1, the reference's recorded trial list (tests/golden/gmm_calibration_ref.npz), `--batch` calls back to back
    speakers   100 000 clips x 1 000 speakers, 100 target clips per speaker (the verifier's matrix: 400 MB)
    rows       1 000 000 windows x 64 speakers, truth uniform over -1 .. 63 (a float scan's matrix: 256 MB)

    python tools/time_calibration.py [--only reference|speakers|rows] [--rounds 5] [--calls 3] [--batch 50]

Scores are normal variates, the targets' shifted up by 2; n_frames uniform over 50 .. 3000 (the three-parameter model).  Per shape
three calls are timed, interleaved within a round, median and minimum over the rounds:
    fit1     a fit of max_iter = 1: the labels' and duration terms' upload, one pass, the solve, the report's way back, the wait
    fit5     a fit of max_iter = 5 (no fit here converges in five passes).  (fit5 - fit1) / 4 is one PASS: the statistics kernel, the
             levels of the tree and the solve kernel.  The matrix is read once per pass: its bytes over that time are printed against
             the 6.3 TB/s a streaming read reaches on this card and the 8 TB/s of the specification; so is the time per trial, whose
             float64 exp, log1p and division are the other candidate for the bound.  A matrix below 256 MiB may be served from the
             Infinity Cache
    apply    `calls` launches back to back with one synchronisation behind the last, host work included; the matrix is read and written
One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_REACHED, HBM_SPEC = 6.3e12, 8.0e12


def _shape(torch, name, gen):
    """-> (scores on the device [T][S], truth int32 [T], n_frames int64 [T])"""
    if name == "reference":
        z = np.load(os.path.join(ROOT, "tests", "golden", "gmm_calibration_ref.npz"))
        return (torch.tensor(z["llr"].astype(np.float32), device="cuda").reshape(-1, 1), np.where(z["label"] == 1, 0, -1).astype(np.intc),
                z["n_frames"].astype(np.int64))
    if name == "speakers":
        T, S = 100000, 1000
        truth = (np.arange(T) // 100).astype(np.intc)
    else:
        T, S = 1000000, 64
        truth = np.random.default_rng(5).integers(-1, S, T).astype(np.intc)
    x = torch.randn((T, S), device="cuda", generator=gen)
    rows = torch.from_numpy(np.flatnonzero(truth >= 0)).cuda()
    x[rows, torch.from_numpy(truth[truth >= 0].astype(np.int64)).cuda()] += 2.0
    return x, truth, np.random.default_rng(6).integers(50, 3001, T).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("reference", "speakers", "rows"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_calibration.py measures on a GPU: none found")
    L, dl = dsp_amd.load(), dsp_amd.lib
    gen = torch.Generator(device="cuda").manual_seed(11)
    cal = dsp_amd.ScoreCalibrator()
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    for name in ([args.only] if args.only else ["reference", "speakers", "rows"]):
        x, truth, n_frames = _shape(torch, name, gen)
        T, S = x.shape
        out = torch.empty_like(x)
        rep, params = dl.CalibrationReport(), dl.Calibration(1.5, -0.5, 0.1)
        calls = args.batch if name == "reference" else args.calls

        def fit(max_iter):
            cfg = dl.CalibrationConfig(0.5, 1e-10, max_iter, 0)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            dl.check(L.dsp_calibration_fit_device(cal._h, x.data_ptr(), T, S, truth.ctypes.data_as(ip), n_frames.ctypes.data_as(lp), C.byref(cfg), None,
                                                  C.byref(rep), st), "dsp_calibration_fit_device")

        def apply():
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            dl.check(L.dsp_calibration_apply_device(cal._h, x.data_ptr(), T, S, n_frames.ctypes.data_as(lp), C.byref(params), out.data_ptr(), st),
                     "dsp_calibration_apply_device")

        def timed(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        fit(100)                                              # warm-up: code objects, the ring, the workspace; and the whole fit, once
        whole = {"status": dl.CAL_STATUS[rep.status], "n_iter": rep.n_iter, "n_rejected": rep.n_rejected, "a": rep.params.a, "b": rep.params.b,
                 "c": rep.params.c, "objective": rep.objective}
        apply()
        fit(5)
        assert rep.status == dl.CAL_MAX_ITER, "a fit converged within five passes: (fit5 - fit1) / 4 is not a pass"
        res = {"fit1": [], "fit5": [], "apply": []}
        for _ in range(args.rounds):
            res["fit1"].append(timed(lambda: fit(1), calls if name == "reference" else 1))
            res["fit5"].append(timed(lambda: fit(5), calls if name == "reference" else 1))
            res["apply"].append(timed(apply, calls))
        med = {k: float(np.median(v)) for k, v in res.items()}
        pass_ms = (med["fit5"] - med["fit1"]) / 4
        line = {"shape": name, "rows": T, "columns": S, "matrix_bytes": T * S * 4, "whole_fit": whole}
        for k, v in res.items():
            line[f"{k}_ms_median"], line[f"{k}_ms_min"] = round(med[k], 4), round(min(v), 4)
        rate, apply_rate = T * S * 4 / (pass_ms * 1e-3), 2 * T * S * 4 / (med["apply"] * 1e-3)
        line.update(pass_ms=round(pass_ms, 4), pass_ps_per_trial=round(pass_ms * 1e9 / (T * S), 3), pass_read_TBps=round(rate / 1e12, 3),
                    pass_share_of_reached=round(rate / HBM_REACHED, 3), pass_share_of_spec=round(rate / HBM_SPEC, 3),
                    apply_TBps=round(apply_rate / 1e12, 3), apply_share_of_reached=round(apply_rate / HBM_REACHED, 3))
        print(json.dumps(line), flush=True)
        del x, out
    cal.close()


if __name__ == "__main__":
    main()
