#!/usr/bin/env python3
"""Timing of the voice activity detector beside the front end it follows, on the same samples, in one process:

    power     Vad.power: the frame-power kernel over 12 500 ragged clips of 0.5 - 1.5 s at 16 kHz, as GB/s of what it must move
              (4 B per sample read + 8 B per row written) against the 8 TB/s peak
    decide    Vad.decide on that power (statistics, levels, flags, records, the kept_offsets download and its one stream wait)
    select    Vad.select of the kept rows of a [rows][13] matrix
    vad       Vad.run + Vad.select, the whole stage
    features  SpeakerFrontEnd.features (MFCC-400 + sliding CMVN) on the same samples: the yardstick, the two alternating

    python tools/time_vad.py [--clips 12500] [--rounds 9] [--calls 5] [--settle-seconds 1.0]

Each figure is the median over the rounds of `calls` calls between two hipEvents, after a settle loop; within a round the workloads
alternate, the order reversed every other round.  The signal is noise at 1e-3 with bursts on half of its stretches (tests/vad_util.py),
so that about half of the rows are kept.  Nothing is gated on these numbers.  One JSON line per workload, then the ratios."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=12500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--settle-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    from tests import vad_util
    if not torch.cuda.is_available():
        raise SystemExit("time_vad.py measures on a GPU: none found")
    n = args.clips
    rng = np.random.default_rng(1234)              # tools/time_mfcc400.py's lengths
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(rng.integers(8000, 24001, n))
    piece = vad_util.signal(7, 1 << 22)            # 4 M samples of the shared signal, repeated
    flat = torch.from_numpy(np.tile(piece, int(off[-1]) // piece.size + 1)[:int(off[-1])].copy()).cuda()
    fe = dsp_amd.SpeakerFrontEnd()
    vad = dsp_amd.Vad(fe.plan, threshold_db=-20.0, context_frames=5, pad_frames=3)
    feats, fo = fe.features(flat, off)
    power = vad.power(flat, off, fo)
    flags, kept, _ = vad.decide(power, fo)
    samples, rows = int(off[-1]), int(fo[-1])

    def whole():
        f, k, _ = vad.run(flat, off, fo)
        return vad.select(feats, f, fo, k)

    work = {"power": lambda: vad.power(flat, off, fo), "decide": lambda: vad.decide(power, fo), "select": lambda: vad.select(feats, flags, fo, kept),
            "vad": whole, "features": lambda: fe.features(flat, off)}
    names = list(work)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.calls

    t_end = time.perf_counter() + args.settle_seconds
    while time.perf_counter() < t_end:             # settle: code objects, the caching allocator, the clocks
        for name in names:
            work[name]()
        torch.cuda.synchronize()
    res = {name: [] for name in names}
    for r in range(args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            res[name].append(timed(work[name]))
    med = {name: float(np.median(v)) for name, v in res.items()}
    for name in names:
        line = {"workload": name, "clips": n, "samples": samples, "rows": rows, "kept_rows": int(kept[-1]), "ms_median": round(med[name], 4),
                "ms_min": round(min(res[name]), 4)}
        if name == "power":
            gbs = (4.0 * samples + 8.0 * rows) / (med[name] * 1e-3) / 1e9
            line["gb_per_s"], line["of_peak"] = round(gbs, 1), round(gbs / PEAK_GBS, 4)
        print(json.dumps(line), flush=True)
    print(json.dumps({"decide_plus_select_ms": round(med["decide"] + med["select"], 4), "vad_over_features": round(med["vad"] / med["features"], 4)}), flush=True)
    vad.close()
    fe.close()


if __name__ == "__main__":
    main()
