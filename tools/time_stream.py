#!/usr/bin/env python3
"""Interleaved timing of one push of a stream session (dsp_stream_push_device: 100 ms of audio for every stream, the new rows, the new
window's scores) against what a caller had to do without sessions for the same result: hold the last frame_length + (window_frames - 1)
hop_length samples of every stream and run dsp_scanner_run_device over them at every push (one window per stream; moving the held
samples along is not even counted).

    python tools/time_stream.py [--streams 1024 16384] [--rounds 7] [--calls 20] [--only-push]

Pushes of 1 600 samples, window_frames / hop_frames 98 / 10, both models.  The first pushes, in which the session's buffers still grow
and no stream holds a window yet, are not timed.  Times are wall-clock per call, host work included (calls issued back to back, one
synchronisation behind the last), medians over the rounds, in ms.  Prints one JSON line per stream count.  --only-push runs nothing
but pushes: the process to put under rocprofv3 --kernel-trace --stats for the split of a push into its launches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WF, HF, FL, H, PUSH = 98, 10, 400, 160, 1600


def _models(dsp_amd):
    g = os.path.join(ROOT, "tests", "golden")
    net = dsp_amd.StopModel(dict(np.load(os.path.join(g, "stop_model.npz"))))
    s = np.load(os.path.join(g, "speaker_gmm_ref.npz"))
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return net, dsp_amd.SpeakerModel(t, u)


def _time(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only-push", action="store_true")
    args = ap.parse_args()
    import torch
    import dsp_amd
    net, spk = _models(dsp_amd)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    for n in args.streams:
        gen = torch.Generator(device="cuda").manual_seed(7)
        chunks = (torch.rand(n * PUSH, device="cuda", generator=gen) * 2 - 1) * 0.3
        co = np.arange(n + 1, dtype=np.int64) * PUSH
        sess = dsp_amd.StreamSession(plan, n, stop=net, speaker=spk, window_frames=WF, hop_frames=HF)
        held_len = FL + (WF - 1) * H
        held = (torch.rand(n * held_len, device="cuda", generator=gen) * 2 - 1) * 0.3
        held_off = dsp_amd.lib.c_offsets(np.arange(n + 1, dtype=np.int64) * held_len)
        sc = dsp_amd.Scanner(plan, stop=net, speaker=spk, window_frames=WF, hop_frames=HF)

        def push():
            return sess.push(chunks, co)

        def push_scores_only():
            return sess.push(chunks, co, want_rows=False)

        def rescan():
            return sc.run(held, held_off)

        for _ in range(12):                      # ten pushes fill the first window; from then on every push completes one per stream
            out = push()
        assert int(out[0][-1]) == 10 * n and int(out[2][-1]) == n
        if args.only_push:
            print(json.dumps({"streams": n, "push_ms": round(_time(torch, push, args.calls * args.rounds), 4)}), flush=True)
            continue
        assert int(rescan()[0][-1]) == n
        push_scores_only()
        res = {"push": [], "push_scores_only": [], "rescan": []}
        for _ in range(args.rounds):
            res["push"].append(_time(torch, push, args.calls))
            res["push_scores_only"].append(_time(torch, push_scores_only, args.calls))
            res["rescan"].append(_time(torch, rescan, args.calls))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({"streams": n, "samples_per_push": PUSH, "window_frames": WF, "hop_frames": HF,
                          "push_ms": round(med["push"], 4), "push_scores_only_ms": round(med["push_scores_only"], 4),
                          "rescan_last_window_ms": round(med["rescan"], 4), "rescan_over_push": round(med["rescan"] / med["push"], 2),
                          "push_ms_range": [round(min(res["push"]), 4), round(max(res["push"]), 4)],
                          "rescan_ms_range": [round(min(res["rescan"]), 4), round(max(res["rescan"]), 4)]}), flush=True)
        sess.close()
        sc.close()
        del chunks, held
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
