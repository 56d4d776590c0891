#!/usr/bin/env python3
"""Interleaved timing of the window scan (dsp_scanner_run_device: one ragged MFCC pass over the recording, then the stop-net and
speaker-LLR scans) against the same windows cut out into a ragged batch of clips and run through the existing per-clip entries
(dsp_classify_signal_batch_ragged_device for P("stop"); dsp_mfcc_clips_ragged_device + dsp_speaker_llr_ragged_device for the LLR).

    python tools/time_scan.py [--rounds 7] [--calls 5] [--cut-max 36000]

Shapes: one hour at 16 kHz with window_frames / hop_frames 98 / 10, 98 / 1 and 500 / 1.  The cut-clip batch of every window of the hop-1
shapes would not fit in HBM (23 GB and 115 GB of samples): there the batch holds the first --cut-max windows and its time is scaled
by windows / cut-max (reported as "extrapolated").  Prints one JSON line per shape; times are medians over the rounds of the mean
per call, in ms."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _models(dsp_amd):
    g = os.path.join(ROOT, "tests", "golden")
    net = dsp_amd.StopModel(dict(np.load(os.path.join(g, "stop_model.npz"))))
    s = np.load(os.path.join(g, "speaker_gmm_ref.npz"))
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return net, dsp_amd.SpeakerModel(t, u)


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
    ap.add_argument("--cut-max", type=int, default=36000)
    ap.add_argument("--seconds", type=int, default=3600)
    args = ap.parse_args()
    import torch
    import dsp_amd
    net, spk = _models(dsp_amd)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    n = args.seconds * 16000
    gen = torch.Generator(device="cuda").manual_seed(7)
    sig = (torch.rand(n, device="cuda", generator=gen) * 2 - 1) * 0.3
    offsets = [0, n]
    rows = 1 + (n - 400) // 160
    for wf, hop in ((98, 10), (98, 1), (500, 1)):
        sc = dsp_amd.Scanner(plan, stop=net, speaker=spk, window_frames=wf, hop_frames=hop)
        wo, prob, mean, label = sc.run(sig, offsets)
        n_win = int(wo[-1])
        k = min(n_win, args.cut_max)
        clip_len = 400 + (wf - 1) * 160
        cut = sig.unfold(0, clip_len, hop * 160)[:k].contiguous().reshape(-1)
        c_off = dsp_amd.lib.c_offsets(np.arange(k + 1, dtype=np.int64) * clip_len)
        mf_out = torch.empty((k * wf, 13), device="cuda")
        # the scan's numbers on the windows the cut batch holds (a consistency check, not the test suite's gate)
        cut_prob = net.classify_signal_ragged(plan, cut, c_off)
        mf, cfo = plan.clips_ragged(cut, c_off, 2**31 - 1, out=mf_out)
        cut_mean, _ = spk.llr_ragged(mf, cfo)
        max_dp = float((cut_prob - prob[:k]).abs().max())
        same_llr = bool(torch.equal(cut_mean, mean[:k]))

        def scan():
            sc.run(sig, offsets)

        def mfcc_only():
            plan.clips_ragged(sig, offsets, 2**31 - 1, out=mf_out if mf_out.shape[0] >= rows else None)

        def cut_batch():
            net.classify_signal_ragged(plan, cut, c_off)
            m2, f2 = plan.clips_ragged(cut, c_off, 2**31 - 1, out=mf_out)
            spk.llr_ragged(m2, f2)

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
        print(json.dumps({"seconds": args.seconds, "window_frames": wf, "hop_frames": hop, "windows": n_win, "rows": rows,
                          "scan_ms": round(med["scan"], 3), "mfcc_pass_ms": round(med["mfcc_pass"], 3),
                          "cut_clips_ms": round(cut_full, 3), "cut_clips_windows_timed": k, "cut_extrapolated": k < n_win,
                          "cut_over_scan": round(cut_full / med["scan"], 2),
                          "scan_ms_range": [round(min(res["scan"]), 3), round(max(res["scan"]), 3)],
                          "check_max_dP_vs_fused_cut": max_dp, "check_llr_equal": same_llr}), flush=True)
        del cut, mf_out, mf
        sc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
