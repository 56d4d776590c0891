#!/usr/bin/env python3
"""Timing of dsp_trials_evaluate_device at three shapes:

    speakers   100 000 clips x 1 000 speakers, 100 target clips per speaker (the verifier's matrix: 400 MB)
    reference  92 x 1, the reference's recorded trial list (tests/golden/gmm_trials_ref.npz), `--batch` calls back to back
    rows       1 000 000 windows x 64 speakers, truth uniform over -1 .. 63 (a float scan's matrix: 256 MB)

    python tools/time_trials.py [--only speakers|reference|rows] [--rounds 5] [--calls 3] [--batch 200] [--thresholds 200]

Scores are normal variates, the targets' shifted up by 2.  Per shape three calls are timed, interleaved within a round, `calls` launches
back to back with one synchronisation behind the last, host work (the labels' upload, the target lists) included; median and minimum
over the rounds per launch:
    sweep    d_sweep_tp / d_sweep_fp alone: passes 1 and 2 -- min / max and class counts, then the histograms -- and the sweep kernel.
             The matrix is read twice: 2 x its bytes over the time is printed against the 6.3 TB/s a streaming read reaches on this
             card and the 8 TB/s of the specification (MI355X HBM3E).  A matrix below 256 MiB may be served from the Infinity Cache
    roc      d_fa_above / d_fa_equal alone: the gather, pass 3 (exact pair counting) and the AUC kernel; the time per pair of a target
             and a non-target (dsp_trials_pairs) is printed in picoseconds
    all      every output
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


def _time(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def _shape(torch, name, gen):
    """-> (scores on the device [T][S], truth int32 [T])"""
    if name == "speakers":
        T, S = 100000, 1000
        truth = (np.arange(T) // 100).astype(np.intc)
    elif name == "rows":
        T, S = 1000000, 64
        truth = np.random.default_rng(5).integers(-1, S, T).astype(np.intc)
    else:
        z = np.load(os.path.join(ROOT, "tests", "golden", "gmm_trials_ref.npz"))
        return torch.tensor(z["llr"].astype(np.float32), device="cuda").reshape(-1, 1), np.where(z["label"] == 1, 0, -1).astype(np.intc)
    x = torch.randn((T, S), device="cuda", generator=gen)
    rows = torch.from_numpy(np.flatnonzero(truth >= 0)).cuda()
    x[rows, torch.from_numpy(truth[truth >= 0].astype(np.int64)).cuda()] += 2.0
    return x, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("speakers", "reference", "rows"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--thresholds", type=int, default=200)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_trials.py measures on a GPU: none found")
    L = dsp_amd.load()
    gen = torch.Generator(device="cuda").manual_seed(11)
    ev = dsp_amd.TrialEvaluator()
    ip = C.POINTER(C.c_int)
    for name in ([args.only] if args.only else ["reference", "speakers", "rows"]):
        x, truth = _shape(torch, name, gen)
        T, S, n = x.shape[0], x.shape[1], args.thresholds
        tp = truth.ctypes.data_as(ip)
        pairs = dsp_amd.lib.check(L.dsp_trials_pairs(tp, T, S), "dsp_trials_pairs")
        n_tgt = int((truth >= 0).sum())
        cols = torch.empty((S + 1, 10), dtype=torch.int64, device="cuda")
        tps, fps = (torch.empty((S + 1, n), dtype=torch.int64, device="cuda") for _ in range(2))
        above, equal = (torch.empty(max(n_tgt, 1), dtype=torch.int32, device="cuda") for _ in range(2))
        cfg = dsp_amd.lib.TrialsConfig(n)

        def launch(c, t, f, a, e):
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            dsp_amd.lib.check(L.dsp_trials_evaluate_device(ev._h, x.data_ptr(), T, S, tp, C.byref(cfg), c, t, f, a, e, st), "dsp_trials_evaluate_device")

        work = {"sweep": lambda: launch(None, tps.data_ptr(), fps.data_ptr(), None, None),
                "roc": lambda: launch(None, None, None, above.data_ptr(), equal.data_ptr()),
                "all": lambda: launch(cols.data_ptr(), tps.data_ptr(), fps.data_ptr(), above.data_ptr(), equal.data_ptr())}
        calls = args.batch if name == "reference" else args.calls
        for fn in work.values():                              # warm-up: code objects, the ring, the workspace
            fn()
        torch.cuda.synchronize()
        res = {key: [] for key in work}
        for _ in range(args.rounds):
            for key, fn in work.items():
                res[key].append(_time(torch, fn, calls))
        c = cols.cpu().numpy().view(np.dtype(dsp_amd.lib.TRIAL_COLUMN_DTYPE)).reshape(-1)[S]
        sweep, roc = float(np.median(res["sweep"])), float(np.median(res["roc"]))
        out = {"shape": name, "rows": T, "columns": S, "thresholds": n, "targets": n_tgt, "pairs": pairs, "matrix_bytes": T * S * 4, "calls_per_round": calls}
        for key in work:
            out[f"{key}_ms_median"], out[f"{key}_ms_min"] = round(float(np.median(res[key])), 4), round(min(res[key]), 4)
        rate = 2 * T * S * 4 / (sweep * 1e-3)
        out.update(sweep_read_TBps=round(rate / 1e12, 3), sweep_share_of_reached=round(rate / HBM_REACHED, 3), sweep_share_of_spec=round(rate / HBM_SPEC, 3),
                   roc_ps_per_pair=round(roc * 1e9 / pairs, 3) if pairs else None, pooled_best_threshold=float(c["best_threshold"]),
                   pooled_best_correct=int(c["best_correct"]), pooled_auc=float(c["auc"]))
        print(json.dumps(out), flush=True)
        del x, cols, tps, fps, above, equal
    ev.close()


if __name__ == "__main__":
    main()
