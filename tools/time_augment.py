#!/usr/bin/env python3
"""Interleaved timing of the clip augmenter (dsp_augment_*) on 1 000 one-second clips at 22 050 Hz (T = 44 frames):

    stft      dsp_stft_ragged_device                       stft2048_kernel
    istft     dsp_istft_ragged_device on that spectrum     istft2048_kernel + istft_gather_kernel
    stretch   dsp_time_stretch_ragged_device, rate 0.8     stft2048 + pvoc + istft2048 + gather (pvoc alone = stretch - stft - istft(T_out))
    noise     dsp_augment_ragged_device, noise ops         finish_kernel
    apply     dsp_augment_ragged_device, train.py's policy on every clip (a third each of stretch, pitch shift, noise)

    python tools/time_augment.py [--clips 1000] [--rounds 7] [--calls 5] [--only STAGE]

The stages are timed in turn within each round (interleaved), `calls` calls back to back with one synchronisation behind the last; the
per-call time is the median over the rounds, host work and the wrapper's output allocation included.  Beside each: the algorithm's
bytes (every input read once, every output written once; the inverse transform's frame workspace, written and read once, is listed
apart as workspace_bytes) and the time those bytes take at the 8 TB/s HBM roofline.  No threshold: nothing earlier exists to compare
with.  --only STAGE runs nothing but that stage's calls: the process to put under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
SR, RATE = 22050, 0.8
STAGES = ("stft", "istft", "stretch", "noise", "apply")
ROW = 1025 * 8


def _make(torch, dsp_amd, n_clips):
    aug = dsp_amd.Augmenter()
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = (torch.rand(n_clips * SR, device="cuda", generator=gen) * 2 - 1) * 0.5
    offs = dsp_amd.lib.c_offsets(np.arange(n_clips + 1, dtype=np.int64) * SR)
    T = dsp_amd.stft_frames(SR)
    T_out, length = dsp_amd.stretch_frames(T, RATE), dsp_amd.stretch_length(SR, RATE)
    spec, fo = aug.stft(x, offs)
    lengths = np.full(n_clips, SR, np.int64)
    noise_ops = dsp_amd.augment.make_ops([dict(clip=c, kind="noise", sigma=0.005) for c in range(n_clips)])
    policy = aug.draw(np.ones(n_clips, np.int32), prob=1.0, seed=1)
    kinds = np.bincount(policy["kind"], minlength=3).tolist()
    runs = {
        "stft": lambda: aug.stft(x, offs),
        "istft": lambda: aug.istft(spec, fo, lengths),
        "stretch": lambda: aug.time_stretch(x, offs, RATE),
        "noise": lambda: aug.apply(x, offs, noise_ops),
        "apply": lambda: aug.apply(x, offs, policy, seed=1),
    }
    n = n_clips
    info = {
        "stft": {"bytes": n * (SR * 4 + T * ROW)},
        "istft": {"bytes": n * (T * ROW + SR * 4), "workspace_bytes": n * 2 * T * 2048 * 4},
        "stretch": {"bytes": n * (SR * 4 + length * 4), "intermediate_bytes": n * (2 * T * ROW + 2 * T_out * ROW + 2 * T_out * 2048 * 4)},
        "noise": {"bytes": n * 2 * SR * 4},
        "apply": {"bytes": int(n * SR * 4 + int(dsp_amd.augment_out_offsets(offs, policy)[-1]) * 4), "ops_stretch_pitch_noise": kinds},
    }
    return runs, info, (aug, x, spec)


def _time(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", choices=STAGES)
    args = ap.parse_args()
    import torch
    import dsp_amd
    if not torch.cuda.is_available():
        raise SystemExit("time_augment.py measures on a GPU: none found")
    runs, info, _keep = _make(torch, dsp_amd, args.clips)
    names = [args.only] if args.only else list(STAGES)
    for name in names:                                   # warm-up: code objects, workspaces, the resamplers of the policy's ratios
        for _ in range(3):
            runs[name]()
    if args.only:
        print(json.dumps({"stage": args.only, "ms": round(_time(torch, runs[args.only], args.rounds * args.calls), 4)}), flush=True)
        return
    res = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            res[name].append(_time(torch, runs[name], args.calls))
    med = {name: float(np.median(res[name])) for name in names}
    for name in names:
        print(json.dumps(dict(info[name], stage=name, clips=args.clips, samples=SR, ms_per_call=round(med[name], 4),
                              ms_range=[round(min(res[name]), 4), round(max(res[name]), 4)],
                              ms_of_bytes_at_8TBps=round(info[name]["bytes"] / HBM_BYTES_PER_S * 1e3, 4))), flush=True)
    print(json.dumps({"stage": "pvoc (derived)", "note": "stretch - stft - istft x T_out / T: not a measurement of the kernel alone",
                      "ms": round(med["stretch"] - med["stft"] - med["istft"] * (dsp_amd.stretch_frames(44, RATE) / 44.0), 4)}), flush=True)


if __name__ == "__main__":
    main()
