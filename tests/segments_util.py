"""The seeded cases that tests/test_segments_cpu.py (on the reference alone) and tests/test_gpu_segments.py (against the library) share.

Scores are a random telegraph signal per column: a hidden on / off state with a mean dwell of 1.5, 8, 100 or 3000 windows, values drawn
from (0.45, 1) while on and from (0, 0.55) while off, so that with on = 0.6 and off = 0.4 all three zones -- at or above `on`, inside
the band, below `off` -- are populated from both sides.  With more than one column a leading column (its own telegraph over the
columns) is lifted by 1 while its state is on, so that DSP_SEG_EXCLUSIVE sees stretches too, and in quiet stretches every column is
squeezed into the band with the leader on top, so that a best column inherits its state.  1 % of the entries are NaN, +inf or
-inf, 2 % exactly `on` and 2 % exactly `off`.  Everything is computed once per (W, S) and handed out read-only."""
import functools
import os
import subprocess

import numpy as np

from tests import segments_ref as R

ON, OFF = np.float32(0.6), np.float32(0.4)
DWELLS = (1.5, 8.0, 100.0, 3000.0)
W_LIST = (1, 2, 3) + tuple(2 ** k + d for k in range(2, 14) for d in (-1, 0, 1))
S_LIST = (1, 3, 64, 65, 130)
MODES = (R.INDEPENDENT, R.EXCLUSIVE)
MG = ((1, 0), (3, 2), (70, 0), (1, 65))          # (min_windows, max_gap)
SEED = 20240


def _telegraph(rng, n, dwell, start):
    flips = rng.random(n) < 1.0 / dwell
    return (np.cumsum(flips) + start) % 2


@functools.lru_cache(maxsize=None)
def case_scores(W, S, salt=0):
    """float32 [W][S], read-only"""
    rng = np.random.default_rng([SEED, W, S, salt])
    x = np.empty((W, S), np.float32)
    z = np.empty((W, S), np.int64)
    for s in range(S):
        dwell = DWELLS[(s + W + salt) % len(DWELLS)]
        z[:, s] = _telegraph(rng, W, dwell, int(rng.integers(2)))
    hi, lo = rng.uniform(0.45, 1.0, (W, S)), rng.uniform(0.0, 0.55, (W, S))
    x[:] = np.where(z == 1, hi, lo)
    if S > 1:
        lead_dwell = DWELLS[(W + salt + 2) % len(DWELLS)]
        lead = np.cumsum(rng.random(W) < 1.0 / lead_dwell) * 7 % S
        rows = np.arange(W)
        lift = z[rows, lead] == 1
        x[rows[lift], lead[lift]] += np.float32(1.0)
        # quiet stretches: every column inside the band, the lifted leader on top of it -- the best column inherits its state
        quiet = _telegraph(rng, W, 16.0, 0) == 1
        x[quiet] = np.float32(0.4) + np.float32(0.09) * x[quiet]
    u = rng.random((W, S))
    x[u < 0.005] = np.nan
    x[(u >= 0.005) & (u < 0.0075)] = np.inf
    x[(u >= 0.0075) & (u < 0.01)] = -np.inf
    x[(u >= 0.01) & (u < 0.03)] = ON
    x[(u >= 0.03) & (u < 0.05)] = OFF
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case_states(W, S, mode, salt=0):
    """uint8 [W][S]: the reference's states of case_scores(W, S, salt), read-only"""
    st = R.all_states(case_scores(W, S, salt), [0, W], ON, OFF, mode)
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def case_ref(W, S, mode, m, g, salt=0):
    """(segments, counts) of the reference for one recording of W windows"""
    return R.segments(case_scores(W, S, salt), [0, W], ON, OFF, m, g, mode, state=case_states(W, S, mode, salt))


# ragged batches: recordings of these W in one call, a recording without windows first, in the middle and last
RAGGED = {
    "small": (0, 1, 63, 0, 64, 65, 2, 0),
    "chunks": (0, 4097, 3, 0, 4095, 129, 0),
    "long": (8193, 0, 1, 4096),
}
RAGGED_S = (1, 3, 65)


@functools.lru_cache(maxsize=None)
def ragged_case(name, S):
    """-> (scores [Wt][S], window_offsets int64): the recordings of RAGGED[name], each its own case_scores (salt = its position)"""
    ws = RAGGED[name]
    parts = [case_scores(W, S, 100 + i) if W else np.zeros((0, S), np.float32) for i, W in enumerate(ws)]
    x = np.concatenate(parts, axis=0)
    x.setflags(write=False)
    return x, np.concatenate(([0], np.cumsum(ws))).astype(np.int64)


def family_facts(S, mode):
    """What the cases of one family -- every W and every (min_windows, max_gap) at one S and mode -- exercise, from the reference alone:
    survivors, merges, drops, survivors that cross a multiple of 64 and of 4096 windows, windows inside the band that inherit state 1."""
    facts = dict(survivors=0, merges=0, drops=0, cross64=0, cross4096=0, inherited=0)
    for W in W_LIST:
        x, st = case_scores(W, S), case_states(W, S, mode)
        e = R.effective(x, mode)
        with np.errstate(invalid="ignore"):
            band = (e >= OFF) & ~(e >= ON)
        facts["inherited"] += int((band & (st == 1)).sum())
        for m, g in MG:
            segs, _ = case_ref(W, S, mode, m, g)
            facts["survivors"] += segs.size
            first, last = segs["first_window"], segs["first_window"] + segs["n_windows"] - 1
            facts["cross64"] += int((first // 64 != last // 64).sum())
            facts["cross4096"] += int((first // 4096 != last // 4096).sum())
            for s in range(S):
                _, merges, drops = R.merge_and_drop(R.runs_of(st[:, s]), m, g)
                facts["merges"] += merges
                facts["drops"] += drops
    return facts


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dsp_amd")


def build_main_segments(out):
    """examples/main_segments.c with gcc, as its header comment shows -> the executable's path"""
    import dsp_amd
    dsp_amd.load()                                  # builds libdsp_amd.so when stale
    cmd = ["gcc", "-O2", "-std=gnu11", "-D__HIP_PLATFORM_AMD__", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
           os.path.join(ROOT, "examples", "main_segments.c"), f"-L{LIBDIR}", "-ldsp_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out


def write_stop_model(path, params):
    """the text file examples/main_segments.c reads: n_coef max_frames units, the scaler, kernel and bias of each layer"""
    units = [int(np.asarray(params[f"bias{l}"]).size) for l in range(4)]
    with open(path, "w") as f:
        f.write(f"{int(params['n_coef']) if 'n_coef' in params else 13} {int(params['max_frames']) if 'max_frames' in params else 500} " + " ".join(map(str, units)) + "\n")
        for key in ["scaler_mean", "scaler_scale"] + [f"{kind}{l}" for l in range(4) for kind in ("kernel", "bias")]:
            f.write(" ".join(repr(float(v)) for v in np.asarray(params[key], np.float32).ravel()) + "\n")
