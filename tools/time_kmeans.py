#!/usr/bin/env python3
"""Interleaved timing of the k-means start of UBM training (dsp_kmeans_*) on the shape of the reference's train_ubm.py:

    2 500 000 rows x 13 coefficients, k = 32

    python tools/time_kmeans.py [--rows 2500000] [--k 32] [--d 13] [--iters 20] [--rounds 5] [--only seed|lloyd|em|small_lloyd|small_em]

Workloads, timed in turn within each round (interleaved):
    seed         UbmTrainer.kmeans_seed: k passes over the rows and k single-block picks; ms per step, and the ratio of a step to the
                 time the rows take at the read-streaming figure of DESIGN.md
    lloyd        UbmTrainer.kmeans for --iters iterations at tol = 0 from the seed rows (the global-variance pass, the final pass and the
                 read-back are in it, once per call: two more passes over the rows, so the figure per iteration is from --iters + 2 passes)
    em           UbmTrainer.fit for --iters iterations at tol = 0 from the k-means start: the yardstick, tools/time_ubm.py's `em` line --
                 a Lloyd pass reads the same bytes and does less arithmetic
    small_lloyd  6 000 rows, 300 iterations: all launches
    small_em     the same for EM
One JSON line per result.  --only runs nothing but that workload: the process to put under rocprofv3 --kernel-trace --stats."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2500000)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--d", type=int, default=13)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["seed", "lloyd", "em", "small_lloyd", "small_em"])
    args = ap.parse_args()
    import torch
    import dsp_amd
    from tests import enroll_ref as E
    if not torch.cuda.is_available():
        raise SystemExit("time_kmeans.py measures on a GPU: none found")
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
    small = feats[:6000].contiguous()
    rows = tr.kmeans_seed(feats, 42)
    centres = feats[torch.from_numpy(rows).cuda()].double().cpu().numpy()
    small_centres = small[torch.from_numpy(small_tr.kmeans_seed(small, 42)).cuda()].double().cpu().numpy()
    start = tr.kmeans(feats, centres, max_iter=args.iters, tol=0.0)
    small_start = small_tr.kmeans(small, small_centres, max_iter=20, tol=0.0)
    work = {"seed": lambda: tr.kmeans_seed(feats, 42),
            "lloyd": lambda: tr.kmeans(feats, centres, max_iter=args.iters, tol=0.0),
            "em": lambda: tr.fit(feats, init=start, max_iter=args.iters, tol=0.0),
            "small_lloyd": lambda: small_tr.kmeans(small, small_centres, max_iter=300, tol=0.0),
            "small_em": lambda: small_tr.fit(small, init=small_start, max_iter=300, tol=0.0)}
    # a Lloyd call stops by itself when no label changes; what it ran is what it is divided by
    ran = {"lloyd": lambda r: r["n_iter"] + 2, "small_lloyd": lambda r: r["n_iter"] + 2}
    per = {"seed": k, "em": args.iters, "small_em": 300}
    names = [args.only] if args.only else list(work)
    for name in names:                                   # warm-up: code objects, workspaces; and how many passes a Lloyd call makes
        out = work[name]()
        if name in ran:
            per[name] = ran[name](out)
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            res[name].append(_time(torch, work[name]) / per[name])
    for name in names:
        med, low = float(np.median(res[name])), float(min(res[name]))
        nrows = 6000 if name.startswith("small") else n
        floor = nrows * d * 4 / HBM_BYTES_PER_S * 1e3
        print(json.dumps({"workload": name, "rows": nrows, "k": k, "d": d, "passes_per_call": per[name], "ms_per_pass_median": round(med, 5),
                          "ms_per_pass_min": round(low, 5), "rows_per_s": round(nrows / (med * 1e-3), 0), "hbm_floor_ms": round(floor, 5),
                          "fraction_of_hbm_floor": round(floor / med, 4)}), flush=True)
    if "lloyd" in res and "em" in res:
        print(json.dumps({"lloyd_over_em": round(float(np.median(res["lloyd"]) / np.median(res["em"])), 4)}), flush=True)


if __name__ == "__main__":
    main()
