#!/usr/bin/env python3
"""Wall-clock timing of the blocking *_host entries -- what a caller who arrives with host memory gets -- for one or more builds of
libdsp_amd.so in ONE process, rounds interleaved (as tools/ab.py does for kernels), from pageable and from pinned input, beside two
yardsticks measured in the same rounds: a plain pinned hipMemcpyAsync of the same bytes (the link's rate on this machine at this
moment) and the device entry alone on resident data.

    python tools/time_host.py [--rounds R] [--scale S] [--shapes a,b,...] [--sweep] [--json out.jsonl] new.so [parent.so ...]

Shapes: clips (12 500 x 16 000 float32), clips_pcm16 (the same clips as int16), frames (1 M x 512), classify (49 152 x 16 000 float32),
classify_f64 (16 384 x 16 000 float64), classify_ragged (the bytes of `classify` in clips of 0.5 - 1.5 s), one_clip_mfcc (compute_mfcc)
and one_clip_classify (classify()).  --scale divides the batch sizes (a quick look).  Per shape, variant and input: median and min ms,
GB/s of input bytes, and that rate as a fraction of the measured link rate; a difference between variants counts when it is above the
spread of the rounds (printed).  --sweep: on the first variant (it must have the host pipeline), pinned input over chunk_bytes 16 .. 256 MB x depth 1 .. 4 and pageable
input by each pageable_mode at the default chunk and depth, for the shapes given.  Entries a variant does not export are reported as missing, not timed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def load(path):
    from dsp_amd import lib as dl
    L = C.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in dl.PROTOTYPES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def has(L, name):
    try:
        getattr(L, name)
        return True
    except AttributeError:
        return False


class Shape:
    """One workload: the host input (pageable numpy + a pinned copy), the output arrays, the call per variant, the device entry"""

    def __init__(self, name, args):
        import torch
        self.name, s = name, max(1, args.scale)
        rng = np.random.default_rng(11)
        self.ragged = None
        if name in ("clips", "clips_pcm16", "one_clip_mfcc"):
            n = 1 if name == "one_clip_mfcc" else 12500 // s
            x = rng.uniform(-1, 1, (n, 16000)).astype(np.float32)
            self.x = np.round(x * 32767).astype(np.int16) if name == "clips_pcm16" else x
            self.out = np.empty((n, 98, 13), np.float32)
        elif name == "frames":
            self.x = rng.uniform(-1, 1, ((1 << 20) // s, 512)).astype(np.float32)
            self.out = np.empty((self.x.shape[0], 13), np.float32)
        elif name in ("classify", "classify_f64", "one_clip_classify"):
            n = 1 if name == "one_clip_classify" else (16384 if name == "classify_f64" else 49152) // s
            self.x = rng.uniform(-0.05, 0.05, (n, 16000)).astype(np.float64 if name == "classify_f64" else np.float32)
            self.out = np.empty(n, np.int32)
        elif name == "classify_ragged":
            total = (49152 // s) * 16000
            lengths = []
            while sum(lengths) < total:
                lengths.append(int(rng.integers(8000, 24001)))
            lengths[-1] -= sum(lengths) - total
            self.ragged = np.concatenate([[0], lengths]).cumsum().astype(np.int64)
            self.x = rng.uniform(-0.05, 0.05, total).astype(np.float32)
            self.out = np.empty(len(lengths), np.int32)
        else:
            raise SystemExit(f"unknown shape {name}")
        self.pinned = torch.from_numpy(self.x).pin_memory()
        self.dev = torch.from_numpy(self.x).cuda()
        self.bytes = self.x.nbytes
        self.plans = {}

    def plan(self, L):
        """an MFCC plan of this variant for the MFCC shapes (kept: plan creation is not what is timed)"""
        from dsp_amd.lib import MfccConfig
        if id(L) not in self.plans:
            cfg = MfccConfig()
            L.dsp_mfcc_default_config(C.byref(cfg))
            if self.name == "frames":
                cfg.frame_length = cfg.hop_length = 512
            h = C.c_void_p()
            assert L.dsp_mfcc_plan_create(C.byref(cfg), 0, C.byref(h)) == 0, L.dsp_last_error()
            self.plans[id(L)] = h
        return self.plans[id(L)]

    def host_call(self, L, pinned):
        """-> a callable that makes the blocking host call once, or None where this variant has no such entry"""
        ptr = self.pinned.data_ptr() if pinned else self.x.ctypes.data
        n, out = self.x.shape[0], self.out.ctypes.data
        lp = C.POINTER(C.c_long)
        if self.name == "clips":
            return lambda: L.dsp_mfcc_clips_host(self.plan(L), ptr, n, 16000, 16000, out, 98)
        if self.name == "clips_pcm16":
            if not has(L, "dsp_mfcc_clips_pcm16_host"):
                return None
            return lambda: L.dsp_mfcc_clips_pcm16_host(self.plan(L), ptr, n, 16000, 16000, 1, 0, out, 98)
        if self.name == "frames":
            return lambda: L.dsp_mfcc_frames_host(self.plan(L), ptr, n, out)
        if self.name == "classify":
            return lambda: L.dsp_classify_batch_host(ptr, n, 16000, 16000, out, None)
        if self.name == "classify_f64":
            return lambda: L.dsp_classify_batch_host_f64(None, ptr, n, 16000, 16000, out, None)
        if self.name == "classify_ragged":
            return lambda: L.dsp_classify_batch_ragged_host(None, ptr, len(self.out), self.ragged.ctypes.data_as(lp), out, None)
        if self.name == "one_clip_mfcc":
            return lambda: L.compute_mfcc(ptr, 16000, out, 98) - 98
        if self.name == "one_clip_classify":
            return lambda: L.dsp_classify(ptr, 16000) * 0
        raise AssertionError(self.name)

    def device_call(self, L):
        """-> a callable that runs the device entry alone on the resident copy and waits for it"""
        import torch
        n, d = self.x.shape[0], self.dev.data_ptr()
        lp = C.POINTER(C.c_long)
        if self.name in ("clips", "clips_pcm16", "one_clip_mfcc", "frames"):
            d_out = torch.empty(self.out.shape, dtype=torch.float32, device="cuda")
        else:
            d_out = torch.empty(len(self.out), dtype=torch.int32, device="cuda")
        o = d_out.data_ptr()
        call = {
            "clips": lambda: L.dsp_mfcc_clips_device(self.plan(L), d, n, 16000, 16000, o, 98, None),
            "one_clip_mfcc": lambda: L.dsp_mfcc_clips_device(self.plan(L), d, 1, 16000, 16000, o, 98, None),
            "clips_pcm16": lambda: L.dsp_mfcc_clips_pcm16_device(self.plan(L), d, n, 16000, 16000, 1, 0, o, 98, None),
            "frames": lambda: L.dsp_mfcc_frames_device(self.plan(L), d, n, o, None),
            "classify": lambda: L.dsp_classify_batch_device(d, n, 16000, 16000, o, None),
            "one_clip_classify": lambda: L.dsp_classify_batch_device(d, 1, 16000, 16000, o, None),
            "classify_f64": lambda: L.dsp_classify_batch_device_f64(None, d, n, 16000, 16000, o, None, None),
            "classify_ragged": lambda: L.dsp_classify_batch_ragged_device(None, d, len(self.out), self.ragged.ctypes.data_as(lp), o, None),
        }[self.name]

        def run():
            rc = call()
            torch.cuda.synchronize()
            return min(rc, 0)
        return run

    def link_call(self):
        """a plain pinned copy of the same bytes to the GPU, waited for"""
        import torch
        dst = torch.empty_like(self.dev)

        def run():
            dst.copy_(self.pinned, non_blocking=True)
            torch.cuda.synchronize()
            return 0
        return run


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t0
    if rc < 0:
        raise SystemExit(f"a timed call failed ({rc})")
    return dt * 1e3


def summarize(ms):
    med = statistics.median(ms)
    return med, min(ms), (max(ms) - min(ms)) / med if med > 0 else 0.0


def run_shape(shape, libs, names, rounds, emit):
    calls = {"link": shape.link_call()}
    for L, tag in zip(libs, names):
        calls[f"{tag}:device"] = shape.device_call(L)
        for pinned in (False, True):
            c = shape.host_call(L, pinned)
            key = f"{tag}:{'pinned' if pinned else 'pageable'}"
            if c is None:
                emit({"shape": shape.name, "case": key, "missing": True})
            else:
                calls[key] = c
    reps = 50 if shape.name.startswith("one_clip") else 1          # a single clip is a fraction of a millisecond: the mean of 50 calls per round
    if reps > 1:
        calls = {k: (lambda c=c: min(c() for _ in range(reps))) for k, c in calls.items()}
    times = {k: [] for k in calls}
    for k, c in calls.items():                   # once untimed: workspaces, rings and plans are made here
        timed(c)
    for _ in range(rounds):
        for k, c in calls.items():
            times[k].append(timed(c) / reps)
    link = statistics.median(times["link"])
    for k, ms in times.items():
        med, lo, spread = summarize(ms)
        emit({"shape": shape.name, "case": k, "bytes": shape.bytes, "median_ms": round(med, 4), "min_ms": round(lo, 4), "spread": round(spread, 4),
              "gb_per_s": round(shape.bytes / med / 1e6, 3), "of_link": round(link / med, 4), "rounds": rounds})


def sweep(shape, L, rounds, emit):
    """pinned input over chunk_bytes x depth; pageable input by each pageable_mode at the library's default chunk and depth"""
    from dsp_amd.lib import HostPipelineConfig
    cfg = HostPipelineConfig()

    def one(call, mb, depth, mode, label):
        cfg.chunk_bytes, cfg.depth, cfg.pageable_mode = mb << 20, depth, mode
        assert L.dsp_host_pipeline_set(0, C.byref(cfg)) == 0
        timed(call)
        med, lo, spread = summarize([timed(call) for _ in range(rounds)])
        emit({"shape": shape.name, "sweep": True, "input": label, "chunk_mb": mb, "depth": depth, "median_ms": round(med, 4),
              "min_ms": round(lo, 4), "spread": round(spread, 4), "gb_per_s": round(shape.bytes / med / 1e6, 3)})

    try:
        assert L.dsp_host_pipeline_get(0, C.byref(cfg)) == 0
        mb0, depth0 = cfg.chunk_bytes >> 20, cfg.depth
        cfg.classify_min_clips = 1                      # the classifiers' chunks as chunk_bytes says
        call = shape.host_call(L, True)
        for mb in (16, 32, 64, 128, 256):
            for depth in (1, 2, 3, 4):
                one(call, mb, depth, 0, "pinned")
        call = shape.host_call(L, False)
        for mode, label in ((0, "pageable, staged"), (1, "pageable, registered"), (2, "pageable, direct"), (3, "pageable, whole")):
            one(call, mb0, depth0, mode, label)
    finally:
        L.dsp_host_pipeline_set(0, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="+", help="path[=name] of a libdsp_amd.so; the first is the build under test")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--shapes", default="clips,clips_pcm16,frames,classify,classify_f64,classify_ragged,one_clip_mfcc,one_clip_classify")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    libs, names = [], []
    for v in args.variants:
        path, _, tag = v.partition("=")
        libs.append(load(path))
        names.append(tag or os.path.basename(os.path.dirname(os.path.abspath(path))) or path)
    out = open(args.json, "a") if args.json else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in args.shapes.split(","):
        shape = Shape(name, args)
        if args.sweep:
            sweep(shape, libs[0], args.rounds, emit)
        else:
            run_shape(shape, libs, names, args.rounds, emit)
        del shape
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
