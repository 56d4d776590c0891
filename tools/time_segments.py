#!/usr/bin/env python3
"""Interleaved timing of dsp_segments_device against the scan that produced its input, at two shapes:

    stop     the stop-word scan of 64 one-hour recordings (359 998 MFCC rows each, window 98, hop 10: 35 991 windows), S = 1
    speakers the float speaker scan of INTEGRATION.md 6i (recordings of 30 000 rows, k 32, d 13), S = 1024

    python tools/time_segments.py [--recordings 64] [--speakers 1024] [--speaker-recordings 3] [--rounds 7] [--calls 3] [--clock-seconds 2]
                                  [--only stop_scan|stop_segments|speakers_scan|speakers_segments]

The scans run on random rows shaped like their inputs (the stop net of the golden fixture, the reference UBM): their cost does not depend
on the values.  The segmenter's does, a little, through the number of runs, so its thresholds are the 60 % and 40 % quantiles of the
scores it is given (of the windows' best LLR under DSP_SEG_EXCLUSIVE at `speakers`), min_windows 3, max_gap 2; the segments found are
printed.  Within each round scan and segmenter alternate; `calls` launches go out back to back with one synchronisation behind the last,
and the per-launch time is the median and the minimum over the rounds, host work included.  The segmenter writes into a buffer of its
capacity and copies nothing to the host.  Printed per shape, one JSON line: both times, the segmenter's share of the scan's, and its
multiple of the time to read the scores once at the rate a large device reduction reaches on this card (measured here, printed).  Then
the box's clock, as tools/time_verify_scan.py prints it.  --only runs nothing but that workload's launches."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_enroll import _clock_under_load, _time, _ubm  # noqa: E402


def _read_rate(torch):
    """bytes per second of a device reduction over 1 GiB (the best of 5)"""
    x = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    best = min(_time(torch, x.sum, 3) for _ in range(5))
    return x.numel() * 4 / (best * 1e-3)


def _segment_call(dsp_amd, torch, seg, scores, wo, on, off, exclusive):
    """-> (a launch of dsp_segments_device into a buffer of the capacity, the device's d_total)"""
    n_col = scores.shape[1] if scores.dim() == 2 else 1
    cfg = dsp_amd.lib.SegmentConfig(on, off, 3, 2, 1 if exclusive else 0)
    lp = C.POINTER(C.c_long)
    room = dsp_amd.segments_capacity(wo, n_col, 3, 2)
    out = torch.empty((room, 8), dtype=torch.int32, device="cuda")
    total = torch.zeros(2, dtype=torch.int64, device="cuda")
    wo = np.ascontiguousarray(wo, np.int64)

    def launch():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        dsp_amd.lib.check(seg._L.dsp_segments_device(seg._h, scores.data_ptr(), wo.size - 1, wo.ctypes.data_as(lp), n_col, C.byref(cfg), out.data_ptr(), room,
                                                     None, total.data_ptr(), st), "dsp_segments_device")
    return launch, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--rows", type=int, default=359998)
    ap.add_argument("--speakers", type=int, default=1024)
    ap.add_argument("--speaker-recordings", type=int, default=3)
    ap.add_argument("--speaker-rows", type=int, default=30000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only")
    ap.add_argument("--clock-seconds", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_segments.py measures on a GPU: none found")
    gen = torch.Generator(device="cuda").manual_seed(7)
    seg = dsp_amd.Segmenter()
    work, shape = {}, {}

    # the stop scan: P(stop) per window, S = 1
    stop = dsp_amd.StopModel(dict(np.load(os.path.join(ROOT, "tests", "golden", "stop_model.npz"))))
    mfcc = 20.0 * torch.randn((args.recordings * args.rows, stop.n_coef), device="cuda", generator=gen)
    fo = np.arange(args.recordings + 1, dtype=np.int64) * args.rows
    wo, prob = stop.scan(mfcc, fo, 98, 10)
    q = torch.quantile(prob[:1 << 20].float(), torch.tensor([0.6, 0.4], device="cuda")).tolist()
    work["stop_scan"] = lambda: stop.scan(mfcc, fo, 98, 10)
    work["stop_segments"], stop_total = _segment_call(dsp_amd, torch, seg, prob, wo, q[0], q[1], False)
    shape["stop"] = {"recordings": args.recordings, "columns": 1, "windows": int(wo[-1]), "score_bytes": int(wo[-1]) * 4}

    # the float speaker scan: LLR per window and speaker
    ubm = _ubm()
    k, d = ubm["means"].shape
    ver = dsp_amd.SpeakerVerifier(ubm)
    feats = torch.randn((args.speaker_recordings * args.speaker_rows, d), device="cuda", generator=gen)
    sfo = np.arange(args.speaker_recordings + 1, dtype=np.int64) * args.speaker_rows
    means = (torch.tensor(np.asarray(ubm["means"], np.float32), device="cuda")[None] + 0.05 * torch.randn((args.speakers, k, d), device="cuda", generator=gen)).contiguous()
    swo = dsp_amd.scan_window_offsets(sfo, 98, 10)
    llr = ver.scan(feats, sfo, means, 98, 10, want=("llr",))["llr"]
    top = llr.max(dim=1).values
    sq = torch.quantile(top[:1 << 20], torch.tensor([0.6, 0.4], device="cuda")).tolist()
    work["speakers_scan"] = lambda: ver.scan(feats, sfo, means, 98, 10, want=("llr",))
    work["speakers_segments"], spk_total = _segment_call(dsp_amd, torch, seg, llr, swo, sq[0], sq[1], True)
    shape["speakers"] = {"recordings": args.speaker_recordings, "columns": args.speakers, "windows": int(swo[-1]), "score_bytes": int(swo[-1]) * args.speakers * 4}

    names = [args.only] if args.only else list(work)
    for name in names:                                   # warm-up: code objects, the span rings, the workspaces
        for _ in range(2):
            work[name]()
    if args.only:
        print(json.dumps({"workload": args.only, "ms": round(_time(torch, work[args.only], args.rounds * args.calls), 4)}), flush=True)
        return
    rate = _read_rate(torch)
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:                               # scan, segments, scan, segments: interleaved
            res[name].append(_time(torch, work[name], args.calls))
    for which, total in (("stop", stop_total), ("speakers", spk_total)):
        s, g = res[f"{which}_scan"], res[f"{which}_segments"]
        read_ms = shape[which]["score_bytes"] / rate * 1e3
        found = total.cpu().tolist()
        print(json.dumps(dict({"shape": which}, **shape[which],
                              **{"segments_found": found[0], "segments_written": found[1],
                                 "scan_ms_median": round(float(np.median(s)), 4), "scan_ms_min": round(min(s), 4),
                                 "segments_ms_median": round(float(np.median(g)), 4), "segments_ms_min": round(min(g), 4),
                                 "segments_over_scan": round(float(np.median(g)) / float(np.median(s)), 5),
                                 "read_GBps_measured": round(rate / 1e9, 1), "read_once_ms": round(read_ms, 5),
                                 "segments_over_read_once": round(float(np.median(g)) / read_ms, 2)})), flush=True)
    if args.clock_seconds > 0:
        from tools.gpu_sensors import Sensors
        sens = Sensors.for_device(0)
        print(json.dumps({"idle": sens.read()}), flush=True)
        for name in names:
            print(json.dumps(dict({"clock_under_load": name}, **_clock_under_load(torch, sens, work[name], args.clock_seconds))), flush=True)


if __name__ == "__main__":
    main()
