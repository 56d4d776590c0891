#!/usr/bin/env python3
"""Timing of dsp_cohort_stats_device and dsp_score_normalize_device beside a torch yardstick on the same tensors:

    rows      a row cohort 10 000 clips x 1 000 cohort speakers: a record per row            top_k 0 and 300
    columns   a column cohort 10 000 cohort clips x 1 000 enrolled speakers: a record per column, the matrix not transposed
                                                                                              top_k 0 and 300
    single    one target speaker, a column cohort of 100 000 clips x 1 (the reference's case) top_k 0 and 300
    apply     S-norm of 10 000 x 1 000 scores from the records of `rows` and `columns`

    python tools/time_snorm.py [--only rows|columns|single|apply] [--rounds 7] [--calls 5]

The yardstick of a statistic is torch.topk(x, k, dim) (top_k = 0: the matrix itself), then .mean(dim) and .std(dim, unbiased=False) in
float32 -- another summation, recorded beside ours and not a gate; that of the apply is 0.5 * ((x - mc) / sc + (x - mr) / sr) in float32
on broadcast tensors.  Within a round the calls are interleaved (ours, the yardstick, ours ...), each timed as `calls` launches back to
back with one synchronisation behind the last, host work included; medians and minima over the rounds.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("rows", "columns", "single", "apply"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_snorm.py measures on a GPU: none found")
    gen = torch.Generator(device="cuda").manual_seed(23)
    norm = dsp_amd.ScoreNormalizer()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    def measure(case, ours, yardstick, extra):
        ours()
        yardstick()                                           # warm-up: code objects, the caching allocator
        res = {"ours": [], "torch": []}
        for _ in range(args.rounds):
            res["ours"].append(timed(ours))
            res["torch"].append(timed(yardstick))
        line = dict(case=case, **extra)
        for key, v in res.items():
            line[f"{key}_ms_median"], line[f"{key}_ms_min"] = round(float(np.median(v)), 4), round(min(v), 4)
        line["ours_over_torch"] = round(line["ours_ms_median"] / line["torch_ms_median"], 3)
        print(json.dumps(line), flush=True)

    def yardstick_stats(x, dim, k):
        top = x if k == 0 else torch.topk(x, k, dim=dim).values
        return top.mean(dim), top.std(dim, unbiased=False)

    shapes = {"rows": (10000, 1000, "row", 1), "columns": (10000, 1000, "column", 0), "single": (100000, 1, "column", 0)}
    for name in ([args.only] if args.only else ["rows", "columns", "single", "apply"]):
        if name == "apply":
            x = torch.randn((10000, 1000), device="cuda", generator=gen) * 0.5 - 0.3
            row = norm.stats(torch.randn((10000, 1000), device="cuda", generator=gen), "row", 300)
            col = norm.stats(torch.randn((10000, 1000), device="cuda", generator=gen), "column", 300)
            r, c = norm.stats_to_numpy(row), norm.stats_to_numpy(col)
            mr, sr = (torch.tensor(r[key].astype(np.float32), device="cuda").reshape(-1, 1) for key in ("mean", "std"))
            mc, sc = (torch.tensor(c[key].astype(np.float32), device="cuda").reshape(1, -1) for key in ("mean", "std"))
            out = torch.empty_like(x)
            measure("apply", lambda: norm.apply(x, "s", row, col, 1e-6, out=out), lambda: 0.5 * ((x - mc) / sc + (x - mr) / sr),
                    dict(rows=10000, columns=1000, mode="s", bytes_moved=2 * x.numel() * 4))
            continue
        R, Cn, axis, dim = shapes[name]
        x = torch.randn((R, Cn), device="cuda", generator=gen) * 0.5 - 0.3
        for k in (0, 300):
            measure(name, lambda: norm.stats(x, axis, k), lambda: yardstick_stats(x, dim, k),
                    dict(rows=R, columns=Cn, axis=axis, top_k=k, matrix_bytes=R * Cn * 4))
        del x
    norm.close()


if __name__ == "__main__":
    main()
