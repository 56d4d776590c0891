#!/usr/bin/env python3
"""Interleaved timing of the scrub-jay scan (dsp_scrubjay_scanner_run_device: one ragged MFCC pass over the recording, the windows'
head rows under stream framing, then svm_scan_kernel) against the same windows cut out into a ragged batch of clips and run through
dsp_scrubjay_fused_ragged_device (ScrubJay.ragged), the per-clip entry each window's results must equal.

    python tools/time_scrubjay_scan.py [--rounds 7] [--calls 5] [--cut-max 20000]

Shapes: one hour at 16 kHz through scrubjay_infer.c's aubio front end (2048 / 1024, stream framing) with window_frames / hop_frames
16 / 4 and 16 / 1, and through the reference's 512-point framing with 20 coefficients (BASELINE config 5) at 98 / 10.  Where a shape
has more windows than --cut-max, the cut-out batch holds the first --cut-max windows and its time is scaled by windows / cut-max
(reported as "extrapolated").  Prints one JSON line per shape; times are medians over the rounds of the mean per call, in ms."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cut-max", type=int, default=20000)
    ap.add_argument("--seconds", type=int, default=3600)
    args = ap.parse_args()
    import torch
    import dsp_amd
    from dsp_amd import scrubjay
    m = np.load(os.path.join(ROOT, "tests", "golden", "scrubjay_svm.npz"))
    attrs = {k: m[k] for k in m.files}
    n = args.seconds * 16000
    gen = torch.Generator(device="cuda").manual_seed(7)
    sig = (torch.rand(n, device="cuda", generator=gen) * 2 - 1) * 0.3
    offsets = [0, n]
    front_ends = {"aubio": scrubjay.scrubjay_infer_config(16000), "512": dsp_amd.default_config(n_mfcc=20)}
    for name, wf, hf in (("aubio", 16, 4), ("aubio", 16, 1), ("512", 98, 10)):
        cfg = front_ends[name]
        sj = scrubjay.ScrubJay(attrs, config=cfg)
        sc = scrubjay.ScrubJayScanner(sj, wf, hf)
        wo, labels, dec, p1, feat = sc.run(sig, offsets)
        n_win = int(wo[-1])
        rows = dsp_amd.frames_for(cfg, n, 2**31 - 1)
        starts, lengths = scrubjay.scan_window_spans(cfg, offsets, wf, hf)
        k = min(n_win, args.cut_max)
        clip_len, step = int(lengths[0]), hf * cfg.hop_length
        assert (lengths[:k] == clip_len).all() and (starts[:k] == np.arange(k) * step).all()
        cut = sig.unfold(0, clip_len, step)[:k].contiguous().reshape(-1)
        c_off = dsp_amd.lib.c_offsets(np.arange(k + 1, dtype=np.int64) * clip_len)
        # the scan's numbers on the windows the cut batch holds (a consistency check, not the test suite's gate)
        cl, cd, cp, cf = sj.ragged(cut, c_off)
        same = bool(torch.equal(cl, labels[:k]) and torch.equal(cd, dec[:k]) and torch.equal(cp, p1[:k]) and torch.equal(cf, feat[:k]))

        def scan():
            sc.run(sig, offsets)

        def mfcc_only():
            sj.plan.clips_ragged(sig, offsets, 2**31 - 1)

        def cut_batch():
            sj.ragged(cut, c_off)

        for fn in (scan, mfcc_only, cut_batch):
            fn()
        torch.cuda.synchronize()
        res = {"scan": [], "mfcc_pass": [], "cut": []}
        for _ in range(args.rounds):
            res["scan"].append(_time(torch, scan, args.calls))
            res["mfcc_pass"].append(_time(torch, mfcc_only, args.calls))
            res["cut"].append(_time(torch, cut_batch, args.calls))
        med = {key: float(np.median(v)) for key, v in res.items()}
        cut_full = med["cut"] * n_win / k
        print(json.dumps({"front_end": name, "seconds": args.seconds, "window_frames": wf, "hop_frames": hf, "windows": n_win, "rows": rows,
                          "scan_ms": round(med["scan"], 3), "mfcc_pass_ms": round(med["mfcc_pass"], 3),
                          "cut_clips_ms": round(cut_full, 3), "cut_clips_windows_timed": k, "cut_extrapolated": k < n_win,
                          "cut_over_scan": round(cut_full / med["scan"], 2),
                          "scan_ms_range": [round(min(res["scan"]), 3), round(max(res["scan"]), 3)],
                          "check_equal_to_cut_clips": same}), flush=True)
        del cut
        sc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
