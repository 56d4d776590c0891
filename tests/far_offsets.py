"""Positions past 2^31 elements and 2^32 bytes in the device entry points that take a stride, an offsets array or a row count
(include/dsp_amd.h: `long` strides, `long` counts, `const long *offsets`): the harness and the table of cases that
tests/test_gpu_far_offsets.py runs on a GPU and that tests/test_far_offsets_cpu.py holds against the header without one.

The library's own workloads (BASELINE config 5: 1.6e10 samples) are larger than anything else in the suite drives, so a 32-bit product
in a kernel (`clip * stride`, `row * d`), in a host rebase (`d_mfcc + frame_offsets[0] * n_coef`), in a span table or in a Python wrapper
would show in no other test.  Here every case runs twice on the same probe clips, in the same order:

  compact  the probes next to each other in a small buffer of their own;
  far      the probes inside one ARENA of zeros, placed so that they start at 0, straddle 2^31 elements, straddle 2^32 elements (4-byte
           and smaller elements) and lie wholly past 2^32 (2^31 for 8-byte elements), the pointer handed to the entry being the
           payload's base -- reached by a far stride, by silent filler clips between the probes, or by a row count.

Asserted: every output of the far call equals the compact call's bit for bit (the suite pins each entry's result for a clip
independently of the batch around it, so the compact call is an exact oracle and no CPU reference is needed); every C name the case
declares was reached (a tap on the ctypes functions, as tests/stream_order.py does it); fillers give finite results (silent MFCC rows:
the rows of a silent clip); strided outputs land at c * out_stride with the sentinel bytes around them untouched; and after the case has
zeroed what it wrote, the whole arena is zero again -- a stray write anywhere in 32 GiB shows.

The arena is ONE torch.zeros of uint8: a guard of 2^31 elements of the widest element (8 bytes: 16 GiB) in front of a payload of
2^32 + SLACK 4-byte elements (= 2^31 + SLACK / 2 8-byte ones).  Guard and payload in front of a probe are there for safety, not for
coverage: an index truncated to 32 bits, signed or unsigned, of elements or of bytes, still lands in mapped zero memory and shows as a
wrong result, never as a fault.

Alignment: far and compact positions of a probe are equal modulo ALIGN = 8 elements (16 bytes for int16, 32 for float, 64 for double)
and the uniform strides are multiples of it, so both calls take the same load path (even strides for MFCC, 16-byte multiples where the
vector path is meant).  Interleaved stereo int16 counts as one 4-byte element per sample frame."""
import ctypes as C
import dataclasses
import time

import numpy as np

B31, B32 = 1 << 31, 1 << 32
ALIGN = 8                                  # elements: see the module's docstring
SLACK = 1 << 23                            # 4-byte elements of payload past 2^32
PAST = 1 << 20                             # elements past the boundary at which a probe "wholly past" it starts
OUT0 = 1 << 19                             # strided outputs live in the arena too, their pointer this many 4-byte elements past the payload's base
GUARD_BYTES = B31 * 8
PAYLOAD_BYTES = (B32 + SLACK) * 4
ARENA_BYTES = GUARD_BYTES + PAYLOAD_BYTES
HEADROOM_BYTES = 4 << 30                   # free HBM asked for beyond the arena (the suite's convention)
SENTINEL = 0x5A
PAD = 64                                   # sentinel elements checked in front of and behind every strided output row
ELEM_BYTES = {"f32": 4, "i16": 2, "i16x2": 4, "f64": 8}
LIMIT_MS = 2000.0                          # an entry of groups C and D whose far call takes longer goes to NOT_REACHED with the time measured


def payload_elements(elem_bytes):
    return PAYLOAD_BYTES // elem_bytes


# ---- positions (plain integers: tests/test_far_offsets_cpu.py checks them without a GPU) ----------------------------------------------

def _near(target, residue, lo, hi):
    """the integer nearest `target` in [lo, hi] that is `residue` modulo ALIGN"""
    best = None
    for v in range(max(lo, target - ALIGN), min(hi, target + ALIGN) + 1):
        if v % ALIGN == residue % ALIGN and (best is None or abs(v - target) < abs(best - target)):
            best = v
    assert best is not None, (target, residue, lo, hi)
    return best


def uniform_layout(n, elem_bytes, geometry):
    """equal clips of n elements -> dict(k, far_stride, compact_stride, far, compact, straddles): clip c at c * stride.
    "straddle": three clips; clip 1 straddles 2^31 and clip 2 straddles 2^32 (8-byte elements: clip 1 straddles 2^30 elements = 2^33
    bytes, clip 2 straddles 2^31).  "past": two clips, clip 1 wholly past 2^32 (8-byte: 2^31) -- a product truncated to 32 bits and then
    widened still points at the right start of a straddling clip, not of this one."""
    assert n >= 4 * ALIGN
    compact = -(-n // ALIGN) * ALIGN
    top = B31 if elem_bytes == 8 else B32
    if geometry == "straddle":
        q = _near(n // 4, 0, ALIGN, n // 2 - 1)                 # clip 2 starts at top - 2 q: 2 q < n
        stride, k = top // 2 - q, 3
        straddles = {1: top // 2, 2: top}
    else:
        assert geometry == "past"
        stride, k, straddles = top + PAST, 2, {}
    return dict(k=k, n=n, far_stride=stride, compact_stride=compact, far=[c * stride for c in range(k)], compact=[c * compact for c in range(k)],
                straddles=straddles, past={1: top} if geometry == "past" else {})


def ragged_layout(n, elem_bytes, max_filler=None):
    """probes of n elements back to back in the compact call [0, n, 2 n, ...]; in the far call probe, filler, probe, filler, probe[, filler,
    probe] (max_filler: every filler cut into clips of at most that many elements): [0, n, 2^31 - n/4, 2^31 + 3n/4, 2^32 - n/2, 2^32 + n/2, 2^32 + PAST, ... + n] for elements of 4 bytes or fewer (the quarter and the
    half moved by less than ALIGN so that every probe keeps its compact position modulo ALIGN), [0, n, 2^31 - n/4, 2^31 + 3n/4, 2^31 + PAST,
    ... + n] for 8-byte ones.  -> dict(far_offsets, compact_offsets, probes (indices into the far clips), far, compact, straddles, past)"""
    assert n >= 4 * ALIGN
    starts, straddles, past = [0], {}, {}
    q = _near(n // 4, -n, 1, n - 1)
    starts.append(B31 - q)
    straddles[1] = B31
    if elem_bytes <= 4:
        r = _near(n // 2, -2 * n, 1, n - 1)
        starts.append(B32 - r)
        straddles[2] = B32
    top = B31 if elem_bytes == 8 else B32
    p = len(starts)
    starts.append(top + _near(PAST, p * n, PAST - ALIGN, PAST + ALIGN))
    past[p] = top
    far_offsets, probes = [], []
    for s in starts:
        assert not far_offsets or s > far_offsets[-1]
        if far_offsets and max_filler:                              # many fillers of a legal length instead of one
            far_offsets += list(range(far_offsets[-1] + max_filler, s, max_filler))
        probes.append(len(far_offsets))
        far_offsets += [s, s + n]
    compact_offsets = [c * n for c in range(len(starts) + 1)]
    return dict(n=n, far_offsets=far_offsets, compact_offsets=compact_offsets, probes=probes, far=starts, compact=compact_offsets[:-1],
                straddles=straddles, past=past)


def rows_layout(width, rows):
    """a row-major float32 matrix [..][width] and probes of `rows` rows each: the probes start at row 0, at the last row that starts before
    element 2^31 (so the probe straddles it), likewise 2^32, and PAST elements beyond 2^32.  -> dict(far_rows, compact_rows, total_rows,
    far, compact (element positions), straddles, past)"""
    assert rows * width >= 2
    first = [0, (B31 - 1) // width - (rows - 1) // 2, (B32 - 1) // width - (rows - 1) // 2, (B32 + PAST) // width + 1]
    far = [r * width for r in first]
    return dict(n=rows * width, rows=rows, width=width, far_rows=first, compact_rows=[c * rows for c in range(4)], total_rows=first[-1] + rows,
                far=far, compact=[c * rows * width for c in range(4)], straddles={1: B31, 2: B32}, past={3: B32})


def rebase_layout(width, rows):
    """the same matrix with frame_offsets[0] > 0: four probes back to back, the first straddling 2^32 -- what an entry that rebases its
    pointers on the host (d_mfcc + frame_offsets[0] * width) is handed"""
    start = rows_layout(width, rows)["far_rows"][2]
    first = [start + c * rows for c in range(4)]
    return dict(n=rows * width, rows=rows, width=width, far_rows=first, compact_rows=[c * rows for c in range(4)], total_rows=first[-1] + rows,
                far=[r * width for r in first], compact=[c * rows * width for c in range(4)], straddles={0: B32}, past={}, rebase=True)


def check_layout(lay, elem_bytes, aligned=True):
    """what tests/test_far_offsets_cpu.py asserts of every declared layout"""
    n, room = lay["n"], payload_elements(elem_bytes)
    assert len(lay["far"]) == len(lay["compact"]) >= 2 and (lay["far"][0] == 0 or lay.get("rebase"))
    for c, (f, s) in enumerate(zip(lay["far"], lay["compact"])):
        assert 0 <= f and f + n <= room, (c, f, n, room)
        if aligned:
            assert (f - s) % ALIGN == 0, (c, f, s)
        if c in lay["straddles"]:
            assert f < lay["straddles"][c] < f + n, (c, f, n)
        if c in lay["past"]:
            assert f >= lay["past"][c] + PAST - ALIGN, (c, f)
    assert lay["straddles"] or lay["past"]
    assert all((f + n <= g) for f, g in zip(lay["far"], lay["far"][1:]))


# ---- the table -------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Case:
    id: str
    names: tuple                 # the C entry points the case reaches
    group: str                   # "A" uniform by stride, "B" ragged with a frame cap, "C" ragged without one, "D" far by count
    elem: str                    # the element of the far input: a key of ELEM_BYTES
    layouts: tuple               # the declared layouts, (layout, aligned) each: what the CPU test checks
    run: object                  # run(ctx, golden) -> dict of outputs of the PROBES (CUDA tensors, numpy arrays, numbers)
    note: str = ""
    geometries: tuple = ()       # the far placements the case runs in; () = those of its group


CASES = []

# entries of groups C and D whose far call was measured above LIMIT_MS on the MI355X: name -> (ms, reason).  Empty: the one call that was
# above it (dsp_speaker_llr_ragged_device behind one filler of 1.6e8 rows, 134 864 ms) has a case with fillers of 65 536 rows instead.
NOT_REACHED = {}

# out of scope: name -> reason
_SCORES = "a score-matrix stage: a reference over 2^31 scores is not cheap, and its rows are not independent of the batch (sweeps, cohort statistics, fits)"
_TRAIN = "a training entry: its result is a statistic of all rows, so a compact call on probes is no oracle for it"
_AUG = "the augmenter: the spectrum of a 2^31-sample clip would be tens of GB"
EXEMPT = {
    "dsp_segments_device": _SCORES, "dsp_trials_evaluate_device": _SCORES, "dsp_calibration_fit_device": _SCORES, "dsp_calibration_apply_device": _SCORES,
    "dsp_cohort_stats_device": _SCORES, "dsp_score_normalize_device": _SCORES,
    "dsp_stop_train_set_device": _TRAIN, "dsp_stop_train_runs_device": _TRAIN, "dsp_ubm_init_rows_device": _TRAIN, "dsp_ubm_train_device": _TRAIN,
    "dsp_kmeans_seed_device": _TRAIN, "dsp_kmeans_fit_device": _TRAIN, "dsp_kmeans_train_ubm_device": _TRAIN, "dsp_svm_train_set_device": _TRAIN,
    "dsp_svm_train_problems_device": _TRAIN, "dsp_svm_platt_fit_device": _TRAIN, "dsp_svm_fit_device": _TRAIN,
    "dsp_stft_ragged_device": _AUG, "dsp_istft_ragged_device": _AUG, "dsp_time_stretch_ragged_device": _AUG, "dsp_augment_ragged_device": _AUG,
    "dsp_vad_decide_ragged_device": "reads float64 power per row, not samples: its frame_offsets index rows of a vector the power entry wrote; the far rows "
                                    "of that chain are reached through dsp_rows_select_ragged_device and dsp_vad_frame_power_ragged_device",
    "dsp_vad_run_ragged_device": "dsp_vad_frame_power_ragged_device and the decision in one call: the far samples are reached through the power entry",
    "dsp_rows_kept_offsets_device": "counts flags per clip and waits: a far row count is reached through dsp_rows_select_ragged_device, which reads the same flags",
    "dsp_stream_resample_finish_device": "takes stream numbers, not positions: `streams` indexes the object's own carry",
}
# (dsp_gather_* and every *_host entry are out of scope too -- RCCL, and pinned host memory of arena size -- and carry no *_device name)


def case(id, names, group, elem, layouts, note="", geometries=()):
    names = (names,) if isinstance(names, str) else tuple(names)

    def register(run):
        CASES.append(Case(id, names, group, elem, tuple(layouts), run, note, tuple(geometries)))
        return run
    return register


def covered():
    out = {}
    for c in CASES:
        for name in c.names:
            out.setdefault(name, []).append(c.id)
    return out


# ---- the arena -------------------------------------------------------------------------------------------------------------------------

class Arena:
    """one allocation of zeros: guard, then payload; views of the payload by element type"""

    def __init__(self, torch):
        self.torch = torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.raw = torch.zeros(ARENA_BYTES, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.alloc_ms = (time.perf_counter() - t0) * 1e3
        self.allocations = 1

    @staticmethod
    def room(torch):
        """(free bytes, needed bytes) by mem_get_info"""
        free, _total = torch.cuda.mem_get_info()
        return int(free), ARENA_BYTES + HEADROOM_BYTES

    def payload(self, elem, shift_bytes=0):
        """the payload from `shift_bytes` on as a 1-D tensor of the element's scalar type (int16 for both PCM layouts)"""
        torch = self.torch
        dt = {"f32": torch.float32, "i16": torch.int16, "i16x2": torch.int16, "f64": torch.float64, "u8": torch.uint8}[elem]
        return self.raw[GUARD_BYTES + shift_bytes:].view(dt)

    def is_zero(self):
        """-> (every byte of guard and payload is zero, milliseconds the scan took)"""
        torch = self.torch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dirty = bool(self.raw.view(torch.int64).any().item())
        return not dirty, (time.perf_counter() - t0) * 1e3

    def free(self):
        self.raw = None
        self.torch.cuda.empty_cache()


# ---- one run of a case: compact or far ---------------------------------------------------------------------------------------------------

def _elem_of(a):
    if isinstance(a, Stereo):
        return "i16x2"
    return {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64", np.dtype(np.int16): "i16"}[a.dtype]


class Stereo(np.ndarray):
    """int16 [..][n][2]: interleaved stereo (a marker type: a mono clip of two samples has the same shape)"""


def stereo(a):
    return np.ascontiguousarray(a, np.int16).view(Stereo)


class Ctx:
    """what a case's run function places its inputs and outputs through; `far` says which of the two calls this is"""

    def __init__(self, torch, arena, far, state, geometry="straddle", stride_error=0, inspect_shift=0, max_clips=None):
        self.torch, self.arena, self.far, self.state, self.geometry = torch, arena, far, state, geometry
        self.stride_error, self.inspect_shift, self.max_clips = stride_error, inspect_shift, max_clips      # the controls of the harness
        self.written, self.outs, self.keep, self.positions, self.checks = [], [], [], [], []

    def once(self, key, make):
        """a handle (plan, model, ...) shared by the compact and the far run of a case"""
        if key not in self.state:
            self.state[key] = make()
        return self.state[key]

    # -- inputs
    def _base(self, elem, elements):
        """a zeroed 1-D tensor of `elements` elements: the arena's payload in a far run, a buffer of its own in a compact one"""
        width = 2 if elem == "i16x2" else 1
        if self.far:
            assert elements * ELEM_BYTES[elem] <= PAYLOAD_BYTES, "a far position past the payload"
            return self.arena.payload(elem)[:elements * width]
        t = self.arena.payload(elem)[:0].new_zeros(elements * width + 2 * ALIGN)      # (same dtype and device)
        self.keep.append(t)
        return t[:elements * width]

    def _put(self, base, elem, start, probe):
        width = 2 if elem == "i16x2" else 1
        src = self.torch.from_numpy(np.ascontiguousarray(np.asarray(probe)).reshape(-1))
        base[start * width:start * width + src.numel()].copy_(src)
        if self.far:
            self.written.append((base, start * width, src.numel()))

    def clips(self, probes):
        """probes: [k'][n] (float32, float64, int16) or stereo([k'][n][2]), k' >= the layout's k -> the strided view [k][n](...) the
        uniform entries take, clip c at c * stride"""
        torch = self.torch
        elem = _elem_of(probes)
        n = probes.shape[1]
        lay = uniform_layout(n, ELEM_BYTES[elem], self.geometry)
        k = min(lay["k"], self.max_clips or lay["k"])
        stride = lay["far_stride"] if self.far else lay["compact_stride"]
        base = self._base(elem, (k - 1) * stride + n)
        for c in range(k):
            self._put(base, elem, c * stride, probes[c])
        self.positions.append([c * stride for c in range(k)])
        passed = stride - self.stride_error if self.far else stride
        if elem == "i16x2":
            return torch.as_strided(base, (k, n, 2), (2 * passed, 2, 1))
        return torch.as_strided(base, (k, n), (passed, 1))

    def ragged(self, probes, max_filler=None):
        """probes: equally long [n] (or stereo [n][2]) arrays, as many as ragged_layout has -> (signal, offsets, idx): the flat buffer the
        ragged entries take, its int64 offsets, and the clips that are probes"""
        elem = _elem_of(probes[0])
        n = probes[0].shape[0]
        lay = ragged_layout(n, ELEM_BYTES[elem], max_filler)
        assert len(probes) >= len(lay["far"])
        probes = probes[:len(lay["far"])]
        if self.far:
            off, idx = lay["far_offsets"], lay["probes"]
        else:
            off, idx = lay["compact_offsets"], list(range(len(probes)))
        base = self._base(elem, off[-1])
        for c, p in zip(idx, probes):
            self._put(base, elem, off[c], p)
        self.positions.append([off[c] for c in idx])
        signal = base.view(-1, 2) if elem == "i16x2" else base
        return signal, np.asarray(off, np.int64), idx

    def matrix(self, width, probes):
        """probes: four float32 [rows][width] -> (matrix [total rows][width], the probes' first rows): rows_layout in a far run, the probes
        back to back in a compact one"""
        rows = probes[0].shape[0]
        lay = rows_layout(width, rows)
        first = lay["far_rows"] if self.far else lay["compact_rows"]
        total = lay["total_rows"] if self.far else 4 * rows
        base = self._base("f32", total * width)
        for r, p in zip(first, probes):
            self._put(base, "f32", r * width, p.astype(np.float32))
        self.positions.append([r * width for r in first])
        return base.view(total, width), list(first)

    def rmatrix(self, width, probes, max_filler=None):
        """probes: four float32 [rows][width] -> (matrix [F][width], frame_offsets, idx): a ragged matrix whose recordings are probe,
        filler, probe, filler, probe, filler, probe at the rows of rows_layout -- or, in the "rebase" geometry, the four probes back to
        back with frame_offsets[0] far into the matrix; compact: back to back from row 0.  max_filler: every filler cut into recordings of
        at most that many rows"""
        rows = probes[0].shape[0]
        lay = rebase_layout(width, rows) if self.geometry == "rebase" else rows_layout(width, rows)
        if not self.far:
            first, fo, idx = lay["compact_rows"], [c * rows for c in range(5)], [0, 1, 2, 3]
        elif self.geometry == "rebase":
            first, fo, idx = lay["far_rows"], [lay["far_rows"][0] + c * rows for c in range(5)], [0, 1, 2, 3]
        else:
            first, fo, idx = lay["far_rows"], [], []
            for r in first:
                if fo and max_filler:                               # many filler recordings of max_filler rows instead of one
                    fo += list(range(fo[-1] + max_filler, r, max_filler))
                idx.append(len(fo))
                fo += [r, r + rows]
        total = fo[-1]
        base = self._base("f32", total * width)
        for r, p in zip(first, probes):
            self._put(base, "f32", r * width, p.astype(np.float32))
        self.positions.append([r * width for r in first])
        return base.view(total, width), np.asarray(fo, np.int64), idx

    # -- strided outputs
    def out(self, k, n_out, in_stride):
        """float32 rows [k][n_out] at c * out_stride, sentinel bytes around them -> (pointer tensor, out_stride).  In a far run the rows lie
        in the arena, OUT0 elements behind the payload's base, the stride being the input's far stride moved to the rows' own alignment."""
        torch = self.torch
        compact = -(-(n_out + 2 * PAD) // ALIGN) * ALIGN
        stride = in_stride if self.far else compact
        shift = OUT0 * 4
        span = (k - 1 + self.inspect_shift) * stride + n_out + PAD
        if self.far:
            base = self.arena.payload("f32", shift - PAD * 4)[:span + PAD]
        else:
            base = torch.empty(span + PAD, dtype=torch.float32, device="cuda")
        rows = [PAD + (c + self.inspect_shift) * stride for c in range(k)]            # where the case will look
        for r in rows:
            base[r - PAD:r + n_out + PAD].view(torch.uint8).fill_(SENTINEL)
            if self.far:
                self.written.append((base, r - PAD, n_out + 2 * PAD))
        if self.far and self.inspect_shift:                                        # the control: the call writes one stride in front of where the case looks
            for c in range(k):
                self.written.append((base, PAD + c * stride, n_out))
        self.outs.append((base, rows, n_out))
        return base[PAD:], stride

    def out_rows(self, i=0):
        """the rows of strided output i as one tensor [k][n_out], after the sentinel check"""
        torch = self.torch
        base, rows, n_out = self.outs[i]
        sent = torch.full((PAD * 4,), SENTINEL, dtype=torch.uint8, device=base.device)
        got = []
        for c, r in enumerate(rows):
            front, back = base[r - PAD:r].view(torch.uint8), base[r + n_out:r + n_out + PAD].view(torch.uint8)
            assert torch.equal(front, sent) and torch.equal(back, sent), f"strided output {i}, row {c}: the sentinel bytes around the row were written"
            row = base[r:r + n_out]
            assert not bool((row.view(torch.uint8) == SENTINEL).all().item()), f"strided output {i}, row {c}: the row still holds the sentinel: it was written elsewhere"
            got.append(row.clone())
        return torch.stack(got)

    # -- fillers
    def finite(self, what, t):
        if t is not None and t.numel() and t.is_floating_point():
            assert bool(self.torch.isfinite(t).all().item()), f"{what}: a filler's result is not finite"

    def same_rows(self, what, t, row):
        """every row of t [..][d] equals `row` bit for bit (the MFCC rows of silence)"""
        if t.numel():
            assert bool((t.view(self.torch.int32) == row.view(self.torch.int32).reshape(1, -1)).all().item()), f"{what}: a silent filler's rows are not the rows of silence"

    def cleanup(self):
        for base, start, count in self.written:
            base[start:start + count].zero_()
        self.written, self.outs, self.keep = [], [], []


class Tap:
    """wraps the ctypes functions `names` of the loaded library: which were called, and the milliseconds of each call with the device
    drained before and after it (the far call's time: host and device)"""

    def __init__(self, torch, lib, names):
        self.torch, self.lib, self.names, self.calls, self.saved = torch, lib, names, [], {}

    def __enter__(self):
        for name in self.names:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def tapped(*args, _fn=fn, _name=name):
                self.torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = _fn(*args)
                self.torch.cuda.synchronize()
                self.calls.append((_name, (time.perf_counter() - t0) * 1e3))
                return rc
            setattr(self.lib, name, tapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def _bytes(x):
    if x is None:
        return b""
    if isinstance(x, dict):
        return b"".join(k.encode() + b"=" + _bytes(x[k]) + b";" for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return b"".join(_bytes(v) + b"," for v in x)
    if hasattr(x, "is_cuda"):
        x = x.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(x)
    return str(a.shape).encode() + str(a.dtype).encode() + a.tobytes()


def _first_difference(a, b):
    """(how many bytes differ, the first positions) of two outputs' bytes, for the message of a failure"""
    if len(a) != len(b):
        return f"{len(a)} bytes against {len(b)}"
    d = np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))
    return f"{d.size} of {len(a)} differ, first at {d[:8].tolist()}"


def run_case(torch, arena, c, golden, geometries=None, stride_error=0, inspect_shift=0, max_clips=None):
    """-> the report lines of the case, one dict per geometry; asserts what the module's docstring states"""
    import dsp_amd.lib as dl
    lib = dl.load()
    reports = []
    state = {}
    for geometry in geometries or c.geometries or (("straddle", "past") if c.group == "A" else ("far",)):
        compact = Ctx(torch, arena, False, state, geometry, max_clips=max_clips)
        want = c.run(compact, golden)
        torch.cuda.synchronize()
        want_bytes = {k: _bytes(v) for k, v in want.items()}
        compact.cleanup()
        far = Ctx(torch, arena, True, state, geometry, stride_error, inspect_shift, max_clips)
        try:
            with Tap(torch, lib, c.names) as tap:
                got = c.run(far, golden)
            torch.cuda.synchronize()
            got_bytes = {k: _bytes(v) for k, v in got.items()}
        finally:
            torch.cuda.synchronize()
            positions = far.positions
            far.cleanup()
        clean, scan_ms = arena.is_zero()
        reached = {name for name, _ in tap.calls}
        assert reached == set(c.names), f"{c.id}: declares {sorted(c.names)}, reaches {sorted(reached)}"
        assert set(got_bytes) == set(want_bytes), c.id
        differ = sorted(k for k in want_bytes if got_bytes[k] != want_bytes[k])
        where = {k: _first_difference(got_bytes[k], want_bytes[k]) for k in differ}
        assert not differ, f"{c.id} ({geometry}): {differ} differs from the compact call (bytes: {where})"
        assert clean, f"{c.id} ({geometry}): the arena is not zero after the case zeroed what it wrote: a stray write"
        reports.append({"case": c.id, "geometry": geometry, "entries": list(c.names), "elem_bytes": ELEM_BYTES[c.elem], "positions": positions,
                        "arena_bytes": ARENA_BYTES, "far_ms": {name: round(max(ms for n2, ms in tap.calls if n2 == name), 3) for name in c.names}, "outputs": sorted(want_bytes), "scan_ms": round(scan_ms, 1)})
    return reports


def line(r):
    pos = "; ".join("[" + ", ".join(str(p) for p in ps) + "]" for ps in r["positions"])
    ms = ", ".join(f"{name} {v:.3f} ms" for name, v in r["far_ms"].items())
    return (f"{r['case']:<40} {r['geometry']:<8} element {r['elem_bytes']} B  at {pos}  arena {r['arena_bytes']} B  far call: {ms}  "
            f"outputs: {', '.join(r['outputs'])}  arena scan {r['scan_ms']:.1f} ms")


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------

def _S():
    from tests import signals
    return signals


def noise(n, seed, level=0.5):
    return (_S().uniform_pm1(int(n), seed) * np.float32(level)).astype(np.float32)


def pcm16(x):
    return np.round(np.asarray(x, np.float64) * 32767.0).astype(np.int16)


def probes_f32(n, seed, k=4):
    """k different clips of n samples: noise, noise with a quiet tail, a chirp, noise with a silent head"""
    x = np.stack([noise(n, seed + i) for i in range(k)])
    x[1, n // 3:] *= np.float32(1e-3)
    x[2] = _S().chirp(n, 300.0, 6000.0)
    if k > 3:
        x[3, :n // 2] = 0.0
    return x


def as_input(x, form):
    """float32 probes [k][n] -> the entry's input format: "f32", "i16" (mono), "ch0" / "avg" (interleaved stereo, the other channel
    another signal) -> (array, stereo_mode)"""
    if form == "f32":
        return x, 0
    if form == "i16":
        return pcm16(x), 0
    assert form in ("ch0", "avg")
    return stereo(np.stack([pcm16(x), pcm16(x[::-1] * np.float32(0.5))], axis=-1)), int(form == "avg")


ELEM_OF_FORM = {"f32": "f32", "i16": "i16", "ch0": "i16x2", "avg": "i16x2", "f64": "f64"}
CLIP = 6129                                    # samples of an MFCC clip: odd, no multiple of a hop, 36 rows of 400 / 160
MAX_FRAMES = 64                                # the frame cap of group B: above every probe's count, and what bounds the work on a filler


def _uniform(n, elem):
    return tuple((uniform_layout(n, ELEM_BYTES[elem], g), True) for g in ("straddle", "past"))


def _ragged(n, elem):
    return ((ragged_layout(n, ELEM_BYTES[elem]), True),)


def _models(ctx, golden):
    def make():
        import dsp_amd
        s = golden("speaker_gmm_ref.npz")
        t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
        u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
        return dsp_amd.MfccPlan(dsp_amd.default_config()), dsp_amd.StopModel(dict(golden("stop_model.npz"))), dsp_amd.SpeakerModel(t, u)
    return ctx.once("models", make)


def _svm_attrs(golden):
    m = golden("scrubjay_svm.npz")
    return {k: m[k] for k in m.files}


def _mfcc_cfg(kind):
    import dsp_amd
    from dsp_amd import scrubjay
    if kind == "512":
        return dsp_amd.default_config()
    if kind == "400":
        return dsp_amd.speaker_config()
    if kind == "1024":
        return dsp_amd.default_config(n_fft=1024, frame_length=1024, hop_length=512, n_mels=128)
    if kind == "2048":
        return scrubjay.scrubjay_infer_config(aubio=False)
    assert kind == "aubio2048"
    return scrubjay.scrubjay_infer_config()


def _plan(ctx, kind):
    import dsp_amd
    return ctx.once(("plan", kind), lambda: dsp_amd.MfccPlan(_mfcc_cfg(kind)))


# ---- group A: uniform batches, far by stride ------------------------------------------------------------------------------------------------

def _mfcc_clips_case(kind, form):
    name = "dsp_mfcc_clips_device" if form == "f32" else "dsp_mfcc_clips_pcm16_device"

    @case(f"A_mfcc_clips_{kind}_{form}", name, "A", ELEM_OF_FORM[form], _uniform(CLIP, ELEM_OF_FORM[form]))
    def run(ctx, golden):
        plan = _plan(ctx, kind)
        x, mode = as_input(probes_f32(CLIP, 100), form)
        view = ctx.clips(x)
        return {"mfcc": plan.clips(view, 1 << 20) if form == "f32" else plan.clips_pcm16(view, 1 << 20, mode)}


for _kind in ("512", "400", "1024", "2048"):
    _mfcc_clips_case(_kind, "f32")
for _kind, _forms in (("512", ("i16", "ch0", "avg")), ("aubio2048", ("i16", "ch0", "avg"))):
    for _form in _forms:
        _mfcc_clips_case(_kind, _form)


def _classify_probes():
    c = _S().classify_cases()
    return np.stack([c[k] for k in ("burst_2k", "jay_like", "scrub_a", "noise")])


def _trace(torch, k, f64):
    import dsp_amd.lib as dl
    size = C.sizeof(dl.ClassifyTraceF64 if f64 else dl.ClassifyTrace)
    return torch.zeros(k * size, dtype=torch.uint8, device="cuda")


def _trace_fields(trace, k):
    """the float64 trace records [k] as their fields: the four padding bytes behind n_midpoints belong to no field and are whatever the
    workspace held"""
    import torch
    rec = trace.view(k, -1)
    assert rec.shape[1] == 8 + 8 * 64 + 8 * 64 * 3
    return {"n_midpoints": rec[:, :4].contiguous().view(torch.int32), "midpoints": rec[:, 8:8 + 512].contiguous().view(torch.float64),
            "sums": rec[:, 520:].contiguous().view(torch.float64)}


def _classify_case(entry, form):
    f64 = entry.endswith("_f64")
    elem = "f64" if form == "f64" else ELEM_OF_FORM[form]

    @case(f"A_{entry[4:]}_{form}", entry, "A", elem, _uniform(16000, elem), note="with trace" if f64 else "")
    def run(ctx, golden):
        import importlib
        import dsp_amd.lib as dl
        torch = ctx.torch
        K = importlib.import_module("dsp_amd.classify")
        L = dl.load()
        clips = _classify_probes()
        if form == "f64":
            x, mode = clips.astype(np.float64), 0
        else:
            x, mode = as_input(clips, form)
        view = ctx.clips(x)
        k, n = view.shape[:2]
        stream = dl.current_stream(view)
        if entry == "dsp_classify_batch_device":
            labels = torch.empty(k, dtype=torch.int32, device="cuda")
            dl.check(L.dsp_classify_batch_device(view.data_ptr(), k, n, view.stride(0), labels.data_ptr(), stream), entry)
            return {"labels": labels}
        if entry == "dsp_classify_batch_device_cfg":
            return {"labels": K.classify_device(view, config=K.CLASSIFY_MICROPHONE)}
        if entry == "dsp_classify_batch_device_ctx":
            class Context(dl.Handle):
                _destroy = "dsp_classify_ctx_destroy"

                def __init__(self):
                    self._create("dsp_classify_ctx_create", 0)
            h = ctx.once("classify_ctx", Context)
            labels = torch.empty(k, dtype=torch.int32, device="cuda")
            dl.check(L.dsp_classify_batch_device_ctx(h._h, None, view.data_ptr(), k, n, view.stride(0), labels.data_ptr(), stream), entry)
            return {"labels": labels}
        if entry == "dsp_classify_batch_pcm16_device":
            return {"labels": K.classify_device_pcm16(view, stereo_mode=mode)}
        labels, trace = torch.empty(k, dtype=torch.int32, device="cuda"), _trace(torch, k, True)
        if entry == "dsp_classify_batch_device_f64":
            dl.check(L.dsp_classify_batch_device_f64(None, view.data_ptr(), k, n, view.stride(0), labels.data_ptr(), trace.data_ptr(), stream), entry)
        else:
            channels, stride = dl.pcm_device(view)
            dl.check(L.dsp_classify_batch_pcm16_device_f64(None, view.data_ptr(), k, n, stride, channels, mode, labels.data_ptr(), trace.data_ptr(), stream), entry)
        return dict(_trace_fields(trace, k), labels=labels)


_classify_case("dsp_classify_batch_device", "f32")
_classify_case("dsp_classify_batch_device_cfg", "f32")
_classify_case("dsp_classify_batch_device_ctx", "f32")
for _form in ("i16", "ch0", "avg"):
    _classify_case("dsp_classify_batch_pcm16_device", _form)
_classify_case("dsp_classify_batch_device_f64", "f64")
for _form in ("i16", "ch0", "avg"):
    _classify_case("dsp_classify_batch_pcm16_device_f64", _form)


def _scrubjay(ctx, golden, kind):
    from dsp_amd import scrubjay
    return ctx.once(("scrubjay", kind), lambda: scrubjay.ScrubJay(_svm_attrs(golden), config=None if kind == "512" else scrubjay.scrubjay_infer_config()))


def _fused(out):
    return dict(zip(("labels", "decision", "prob1", "feat"), out))


def _fused_case(kind, form):
    name = "dsp_scrubjay_fused_device" if form == "f32" else "dsp_scrubjay_fused_pcm16_device"

    @case(f"A_scrubjay_fused_{kind}_{form}", name, "A", ELEM_OF_FORM[form], _uniform(CLIP, ELEM_OF_FORM[form]))
    def run(ctx, golden):
        sj = _scrubjay(ctx, golden, kind)
        x, mode = as_input(probes_f32(CLIP, 200), form)
        view = ctx.clips(x)
        return _fused(sj(view) if form == "f32" else sj.pcm16(view, stereo_mode=mode))


for _kind in ("512", "2048"):
    for _form in ("f32", "i16", "ch0", "avg"):
        _fused_case(_kind, _form)


def _signal_case(form):
    name = "dsp_classify_signal_batch_device" if form == "f32" else "dsp_classify_signal_batch_pcm16_device"

    @case(f"A_classify_signal_{form}", name, "A", ELEM_OF_FORM[form], _uniform(16000, ELEM_OF_FORM[form]))
    def run(ctx, golden):
        plan, stop, _spk = _models(ctx, golden)
        x, mode = as_input(probes_f32(16000, 300), form)
        view = ctx.clips(x)
        return {"prob": stop.classify_signal_batch(plan, view) if form == "f32" else stop.classify_signal_batch_pcm16(plan, view, mode)}


for _form in ("f32", "i16", "ch0", "avg"):
    _signal_case(_form)


UPSAMPLE_IN, UPSAMPLE_OUT = 1000, 2205


@case("A_upsample_linear", "dsp_upsample_linear_device", "A", "f32", _uniform(UPSAMPLE_IN, "f32") + _uniform(UPSAMPLE_OUT, "f32"),
      note="stride and out_stride both far: the rows land in the arena")
def _(ctx, golden):
    import dsp_amd.lib as dl
    view = ctx.clips(probes_f32(UPSAMPLE_IN, 400))
    k = view.shape[0]
    lay = uniform_layout(UPSAMPLE_OUT, 4, ctx.geometry)
    out, out_stride = ctx.out(k, UPSAMPLE_OUT, lay["far_stride"])
    dl.check(dl.load().dsp_upsample_linear_device(view.data_ptr(), k, UPSAMPLE_IN, view.stride(0), out.data_ptr(), UPSAMPLE_OUT, out_stride,
                                                   dl.current_stream(view)), "dsp_upsample_linear_device")
    return {"out": ctx.out_rows()}


RESAMPLE_IN = 4411


def _resample_clips_case(form):
    name = "dsp_resample_clips_device" if form == "f32" else "dsp_resample_clips_pcm16_device"
    n_out = -(-RESAMPLE_IN * 160 // 441)

    @case(f"A_resample_clips_{form}", name, "A", ELEM_OF_FORM[form], _uniform(RESAMPLE_IN, ELEM_OF_FORM[form]) + _uniform(n_out, "f32"),
          note="stride and out_stride both far: the rows land in the arena")
    def run(ctx, golden):
        import dsp_amd.lib as dl
        from dsp_amd import resample
        rs = ctx.once("resampler", lambda: resample.Resampler(44100, 16000))
        assert rs.out_samples(RESAMPLE_IN) == n_out
        x, mode = as_input(probes_f32(RESAMPLE_IN, 500), form)
        view = ctx.clips(x)
        k = view.shape[0]
        out, out_stride = ctx.out(k, n_out, uniform_layout(n_out, 4, ctx.geometry)["far_stride"])
        L, stream = dl.load(), dl.current_stream(view)
        if form == "f32":
            got = dl.check(L.dsp_resample_clips_device(rs._h, view.data_ptr(), k, RESAMPLE_IN, view.stride(0), out.data_ptr(), out_stride, stream), name)
        else:
            channels, stride = dl.pcm_device(view)
            got = dl.check(L.dsp_resample_clips_pcm16_device(rs._h, view.data_ptr(), k, RESAMPLE_IN, stride, channels, mode, out.data_ptr(), out_stride, stream), name)
        assert got == n_out
        return {"out": ctx.out_rows()}


for _form in ("f32", "i16", "ch0", "avg"):
    _resample_clips_case(_form)


# ---- group B: ragged sample entries with a frame cap, far by silent filler clips ------------------------------------------------------------

def _take(t, fo, idx):
    """the rows [fo[c], fo[c + 1]) of the clips idx, back to back"""
    return [t[int(fo[c]):int(fo[c + 1])] for c in idx]


def _others(n, idx):
    return [c for c in range(n) if c not in idx]


def _mfcc_ragged_case(kind, form):
    name = "dsp_mfcc_clips_ragged_device" if form == "f32" else "dsp_mfcc_clips_ragged_pcm16_device"

    @case(f"B_mfcc_ragged_{kind}_{form}", name, "B", ELEM_OF_FORM[form], _ragged(CLIP, ELEM_OF_FORM[form]))
    def run(ctx, golden):
        plan = _plan(ctx, kind)
        x, mode = as_input(probes_f32(CLIP, 600), form)
        signal, off, idx = ctx.ragged(list(x))
        mfcc, fo = plan.clips_ragged(signal, off, MAX_FRAMES, mode)
        if ctx.far:
            zeros = signal[:4 * CLIP].clone().zero_()                       # the rows of a silent clip, from a call of its own
            silent, _ = plan.clips_ragged(zeros, np.array([0, 4 * CLIP]), 1, mode)
            for c in _others(off.size - 1, idx):
                rows = mfcc[int(fo[c]):int(fo[c + 1])]
                assert rows.shape[0] == MAX_FRAMES
                ctx.same_rows(f"filler {c}", rows, silent[0])
                if plan.cfg.log_mode == 0:
                    assert not bool(rows.any().item()), f"filler {c}: silence gives exact zeros in the per-frame log mode"
        return {"rows": _take(mfcc, fo, idx), "frames": np.diff(fo)[idx]}


for _kind in ("512", "400", "2048"):
    _mfcc_ragged_case(_kind, "f32")
for _form in ("i16", "ch0", "avg"):
    _mfcc_ragged_case("512", _form)
_mfcc_ragged_case("aubio2048", "i16")


def _fused_ragged_case(kind, form):
    name = "dsp_scrubjay_fused_ragged_device" if form == "f32" else "dsp_scrubjay_fused_ragged_pcm16_device"

    @case(f"B_scrubjay_fused_ragged_{kind}_{form}", name, "B", ELEM_OF_FORM[form], _ragged(CLIP, ELEM_OF_FORM[form]))
    def run(ctx, golden):
        sj = _scrubjay(ctx, golden, kind)
        x, mode = as_input(probes_f32(CLIP, 700), form)
        signal, off, idx = ctx.ragged(list(x))
        out = _fused(sj.ragged(signal, off, MAX_FRAMES, mode))
        rest = _others(off.size - 1, idx)
        for key, t in out.items():
            ctx.finite(f"fillers, {key}", t[rest])
        return {key: t[idx] for key, t in out.items()}


for _kind in ("512", "2048"):
    for _form in ("f32", "i16", "avg"):
        _fused_ragged_case(_kind, _form)


def _signal_ragged_case(form):
    name = "dsp_classify_signal_batch_ragged_device" if form == "f32" else "dsp_classify_signal_batch_ragged_pcm16_device"

    @case(f"B_classify_signal_ragged_{form}", name, "B", ELEM_OF_FORM[form], _ragged(16001, ELEM_OF_FORM[form]), note="the model's own cap of 500 frames")
    def run(ctx, golden):
        plan, stop, _spk = _models(ctx, golden)
        x, mode = as_input(probes_f32(16001, 800), form)
        signal, off, idx = ctx.ragged(list(x))
        prob = stop.classify_signal_ragged(plan, signal, off, mode)
        ctx.finite("fillers, prob", prob[_others(off.size - 1, idx)])
        return {"prob": prob[idx]}


for _form in ("f32", "i16", "ch0", "avg"):
    _signal_ragged_case(_form)


# ---- group D: far by count -------------------------------------------------------------------------------------------------------------------

def _frames_layout(frame_length):
    return ((rows_layout(frame_length, 3), False),)


def _frames_case(kind, frame_length):
    @case(f"D_mfcc_frames_{kind}_frame{frame_length}", "dsp_mfcc_frames_device", "D", "f32", _frames_layout(frame_length),
          note="the headline kernel: 2^22 + 64 frames of 512, or frames of 400 one of which straddles the boundary")
    def run(ctx, golden):
        import dsp_amd
        plan = ctx.once(("frames_plan", kind, frame_length), lambda: dsp_amd.MfccPlan(
            dsp_amd.default_config(frame_length=frame_length, hop_length=frame_length) if kind == "512" else dsp_amd.speaker_config(framing=0)))
        assert plan.cfg.frame_length == frame_length
        x = probes_f32(3 * frame_length, 900).reshape(4, 3, frame_length)
        frames, first = ctx.matrix(frame_length, list(x))
        out = plan.frames(frames)
        ctx.finite("every row", out)
        if ctx.far and plan.cfg.log_mode == 0:
            for a, b in zip(first, first[1:]):
                assert not bool(out[a + 3:b].any().item()), "silent frames give exact zeros in the per-frame log mode"
        return {"rows": [out[r:r + 3] for r in first]}


_frames_case("512", 512)
_frames_case("512", 400)
_frames_case("400", 400)


def _rows(n, d, seed, scale=8.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(np.float32)


def _matrix_layouts(width, rows, rebase=False):
    return ((rows_layout(width, rows), False),) + (((rebase_layout(width, rows), False),) if rebase else ())


def _by_count_case(id, name, t, d, call, scale=8.0):
    """n_clips x t x d crosses 2^31: clips of t rows of d coefficients, three probe clips at each position, silent clips between them"""
    @case(f"D_{id}", name, "D", "f32", _matrix_layouts(t * d, 3))
    def run(ctx, golden):
        x = _rows(4 * 3 * t, d, 1000 + t, scale).reshape(4, 3, t * d)
        m, first = ctx.matrix(t * d, list(x))
        out = call(ctx, golden, m.view(m.shape[0], t, d))
        for key, v in out.items():
            ctx.finite(f"every clip, {key}", v)
        return {key: [v[r:r + 3] for r in first] for key, v in out.items()}


_by_count_case("stop_predict", "dsp_stop_predict_device", 98, 13, lambda ctx, golden, m: {"prob": _models(ctx, golden)[1].predict(m)})
_by_count_case("speaker_llr", "dsp_speaker_llr_device", 37, 13,
               lambda ctx, golden, m: dict(zip(("mean", "label", "ll_target", "ll_ubm"), _models(ctx, golden)[2].llr(m, per_frame=True))), 3.0)


def _mfcc_stats(ctx, golden, m):
    from dsp_amd import scrubjay
    return {"feat": scrubjay.mfcc_stats(m)}


_by_count_case("mfcc_stats", "dsp_mfcc_stats_device", 3, 20, _mfcc_stats)      # (7.2e7 clips of three frames: more than 2^32 / 64 blocks of one clip)


def _svm_predict(ctx, golden, m):
    from dsp_amd import scrubjay
    svm = ctx.once("svm", lambda: scrubjay.SvmModel(_svm_attrs(golden)))
    return dict(zip(("labels", "decision", "prob1"), svm.predict(m.view(m.shape[0], 40))))


# 1.07e8 feature rows.  The first run of this case failed: one block of 64 lanes per row is more than 2^32 work-items, which the runtime
# counted modulo 2^32, and the rows past 4.0e7 were never computed (svm_kernels.hip now walks rows with a bounded grid).
_by_count_case("svm_predict", "dsp_svm_predict_device", 1, 40, _svm_predict, 1.0)

RECORDING = 150                                 # rows of a probe recording of the ragged matrices: above a window of 98 rows, half a CMVN window


def _ragged_matrix_case(id, name, d, call, scale=8.0, rows=RECORDING, max_filler=None, note=""):
    """a ragged matrix [F][d] whose recordings are probe, filler, probe, ... (the fillers ~1.6e8 silent rows each), and the same probes
    back to back behind frame_offsets[0] > 0.  call(ctx, golden, matrix, frame_offsets, idx) -> the probes' outputs"""
    @case(f"D_{id}", name, "D", "f32", _matrix_layouts(d, rows, True), note=note, geometries=("far", "rebase"))
    def run(ctx, golden):
        x = _rows(4 * rows, d, 1100 + d, scale).reshape(4, rows, d)
        m, fo, idx = ctx.rmatrix(d, list(x), max_filler)
        return call(ctx, golden, m, fo, idx)


def _speaker_llr_ragged(ctx, golden, m, fo, idx):
    mean, label, lt, lu = _models(ctx, golden)[2].llr_ragged(m, fo, per_frame=True)
    return {"mean": mean[idx], "label": label[idx], "ll_target": _take(lt, fo, idx), "ll_ubm": _take(lu, fo, idx)}


_ragged_matrix_case("speaker_llr_ragged", "dsp_speaker_llr_ragged_device", 13, _speaker_llr_ragged, 3.0, max_filler=1 << 16,
                    note="fillers of 65 536 rows: the entry walks a clip's rows in sequence, and with one filler of 1.6e8 rows the far call was measured at 134 864 ms")


def _windows(fo, window, hop):
    from dsp_amd import consumers
    return consumers.scan_window_offsets(fo, window, hop)


def _stop_scan(ctx, golden, m, fo, idx):
    wo, prob = _models(ctx, golden)[1].scan(m, fo, 98, 10)
    ctx.finite("every window", prob)
    return {"prob": _take(prob, wo, idx), "windows": np.diff(wo)[idx]}


def _speaker_scan(ctx, golden, m, fo, idx):
    wo, mean, label = _models(ctx, golden)[2].scan(m, fo, 98, 10)
    return {"mean": _take(mean, wo, idx), "label": _take(label, wo, idx), "windows": np.diff(wo)[idx]}


def _svm_scan(ctx, golden, m, fo, idx):
    from dsp_amd import scrubjay
    svm = ctx.once("svm", lambda: scrubjay.SvmModel(_svm_attrs(golden)))
    wo, labels, dec, p1, feat = svm.scan(m, fo, 16, 16)
    return {"labels": _take(labels, wo, idx), "decision": _take(dec, wo, idx), "prob1": _take(p1, wo, idx), "feat": _take(feat, wo, idx), "windows": np.diff(wo)[idx]}


_ragged_matrix_case("stop_scan", "dsp_stop_scan_device", 13, _stop_scan)
_ragged_matrix_case("speaker_scan", "dsp_speaker_scan_device", 13, _speaker_scan, 3.0)
_ragged_matrix_case("svm_scan", "dsp_svm_scan_device", 20, _svm_scan)


def _sweep():
    from tests import verify_util
    return verify_util.sweep_case(5, 13)


def _cmvn(ctx, golden, m, fo, idx):
    import dsp_amd
    z = ctx.once("cmvn", lambda: dsp_amd.Cmvn(13, 300)).apply(m, fo)
    return {"z": _take(z, fo, idx)}


def _enroll(ctx, golden, m, fo, idx):
    import dsp_amd
    out = ctx.once("enroller", lambda: dsp_amd.SpeakerEnroller(_sweep()["ubm"])).enroll(m, fo)
    for key, v in out.items():
        ctx.finite(f"every speaker, {key}", v)
    return {key: v[idx] for key, v in out.items()}


def _verify(ctx, golden, m, fo, idx):
    import dsp_amd
    torch = ctx.torch
    means = torch.from_numpy(np.array(_sweep()["means"][:5])).cuda()
    out = ctx.once("verifier", lambda: dsp_amd.SpeakerVerifier(_sweep()["ubm"])).verify(m, fo, means, want=("llr", "ll_ubm", "ll_target", "best", "best_llr"))
    for key, v in out.items():
        ctx.finite(f"every clip, {key}", v)
    return {key: v[idx] for key, v in out.items()}


def _float_scan(ctx, golden, m, fo, idx):
    import dsp_amd
    torch = ctx.torch
    means = torch.from_numpy(np.array(_sweep()["means"][:5])).cuda()
    out = ctx.once("verifier", lambda: dsp_amd.SpeakerVerifier(_sweep()["ubm"])).scan(m, fo, means, 30, 7, want=("llr", "ll_ubm", "ll_target", "best", "best_llr"))
    wo = _windows(fo, 30, 7)
    return dict({key: _take(v, wo, idx) for key, v in out.items()}, windows=np.diff(wo)[idx])


_ragged_matrix_case("cmvn_ragged", "dsp_cmvn_ragged_device", 13, _cmvn)
_ragged_matrix_case("speaker_enroll_ragged", "dsp_speaker_enroll_ragged_device", 13, _enroll, 1.0)
_ragged_matrix_case("speaker_verify_ragged", "dsp_speaker_verify_ragged_device", 13, _verify, 1.0)
_ragged_matrix_case("speaker_float_scan", "dsp_speaker_float_scan_device", 13, _float_scan, 1.0)


def _rows_select(ctx, golden, m, fo, idx):
    import dsp_amd
    torch = ctx.torch
    vad = ctx.once("vad", lambda: dsp_amd.Vad(dsp_amd.speaker_config()))
    rng = np.random.default_rng(1200)
    flags = torch.zeros(int(fo[-1]), dtype=torch.uint8, device="cuda")              # the fillers keep no row
    kept = np.zeros(fo.size, np.int64)
    for c in idx:
        f = (rng.random(int(fo[c + 1] - fo[c])) < 0.6).astype(np.uint8)
        flags[int(fo[c]):int(fo[c + 1])] = torch.from_numpy(f).cuda()
        kept[c + 1] = f.sum()
    kept = np.cumsum(kept)
    rows, index = vad.select(m, flags, fo, kept, index=True)
    return {"rows": _take(rows, kept, idx), "index": [index[int(kept[c]):int(kept[c + 1])] - int(fo[c]) for c in idx], "kept": np.diff(kept)[idx]}


_ragged_matrix_case("rows_select_ragged", "dsp_rows_select_ragged_device", 13, _rows_select)


# ---- group C: ragged entries without a cap, far by silent fillers of legal length ----------------------------------------------------------------

CLASSIFY_FILLER = 256 + 956 * 224             # 957 spectrogram columns: the longest clip the classifiers take (13.4 s)


def _classify_ragged_case(entry, form):
    f64 = entry.endswith("_f64")
    elem = "f64" if form == "f64" else ELEM_OF_FORM[form]

    @case(f"C_{entry[4:]}_{form}", entry, "C", elem, ((ragged_layout(16000, ELEM_BYTES[elem], CLASSIFY_FILLER), True),),
          note="~20 000 silent fillers of 957 spectrogram columns each (8-byte samples: ~10 000)" + (", with trace" if f64 else ""))
    def run(ctx, golden):
        import importlib
        import dsp_amd.lib as dl
        torch = ctx.torch
        K = importlib.import_module("dsp_amd.classify")
        L = dl.load()
        clips = _classify_probes()
        if form == "f64":
            x, mode = clips.astype(np.float64), 0
        else:
            x, mode = as_input(clips, form)
        signal, off, idx = ctx.ragged(list(x), CLASSIFY_FILLER)
        try:
            if not f64:
                labels = K.classify_device_ragged(signal, off, stereo_mode=mode)
                return {"labels": labels[idx]}
            n = off.size - 1
            co, _n = dl.c_offsets(off)
            labels, trace = torch.empty(n, dtype=torch.int32, device="cuda"), _trace(torch, n, True)
            if form == "f64":
                dl.check(L.dsp_classify_batch_ragged_device_f64(None, signal.data_ptr(), n, co, labels.data_ptr(), trace.data_ptr(), dl.current_stream(signal)), entry)
            else:
                dl.check(L.dsp_classify_batch_ragged_pcm16_device_f64(None, signal.data_ptr(), n, co, signal.dim(), mode, labels.data_ptr(), trace.data_ptr(),
                                                                      dl.current_stream(signal)), entry)
            return dict({key: v[idx] for key, v in _trace_fields(trace, n).items()}, labels=labels[idx])
        finally:
            if ctx.far:                                       # the grow-only workspaces of ~20 000 long clips go back
                torch.cuda.synchronize()
                (K.classify_release_f64 if f64 else K.classify_release)(0)


_classify_ragged_case("dsp_classify_batch_ragged_device", "f32")
for _form in ("i16", "avg"):
    _classify_ragged_case("dsp_classify_batch_ragged_pcm16_device", _form)
_classify_ragged_case("dsp_classify_batch_ragged_device_f64", "f64")
for _form in ("i16", "avg"):
    _classify_ragged_case("dsp_classify_batch_ragged_pcm16_device_f64", _form)


def _resample_ragged_case(form):
    name = "dsp_resample_ragged_device" if form == "f32" else "dsp_resample_ragged_pcm16_device"

    @case(f"C_resample_ragged_{form}", name, "C", ELEM_OF_FORM[form], _ragged(RESAMPLE_IN, ELEM_OF_FORM[form]), note="fillers of just under 2^31 samples, the longest recording")
    def run(ctx, golden):
        from dsp_amd import resample
        rs = ctx.once("resampler", lambda: resample.Resampler(44100, 16000))
        x, mode = as_input(probes_f32(RESAMPLE_IN, 1300), form)
        signal, off, idx = ctx.ragged(list(x))
        out, oo = rs.ragged(signal, off, mode)
        for c in _others(off.size - 1, idx):
            assert not bool(out[int(oo[c]):int(oo[c + 1])].any().item()), f"filler {c}: silence resamples to zeros"
        return {"out": _take(out, oo, idx), "lengths": np.diff(oo)[idx]}


for _form in ("f32", "i16", "avg"):
    _resample_ragged_case(_form)


@case("C_vad_frame_power_ragged", "dsp_vad_frame_power_ragged_device", "C", "f32", _ragged(CLIP, "f32"))
def _(ctx, golden):
    import dsp_amd
    cfg = dsp_amd.speaker_config()
    vad = ctx.once("vad", lambda: dsp_amd.Vad(cfg))
    signal, off, idx = ctx.ragged(list(probes_f32(CLIP, 1400)))
    fo = dsp_amd.mfcc.ragged_frame_offsets(cfg, off, 1 << 30)
    power = vad.power(signal, off, fo)
    for c in _others(off.size - 1, idx):
        assert not bool(power[int(fo[c]):int(fo[c + 1])].any().item()), f"filler {c}: silence has no power"
    return {"power": _take(power, fo, idx), "frames": np.diff(fo)[idx]}


SCAN_CLIP = 24001                              # samples of a scanned probe recording: 148 rows of 400 / 160, six windows of 98 rows every 10


def _scanner_case(form):
    name = "dsp_scanner_run_device" if form == "f32" else "dsp_scanner_run_pcm16_device"

    @case(f"C_scanner_run_{form}", name, "C", ELEM_OF_FORM[form], _ragged(SCAN_CLIP, ELEM_OF_FORM[form]))
    def run(ctx, golden):
        import dsp_amd
        plan, stop, spk = _models(ctx, golden)
        sc = ctx.once("scanner", lambda: dsp_amd.Scanner(plan, stop=stop, speaker=spk, window_frames=98, hop_frames=10))
        x, mode = as_input(probes_f32(SCAN_CLIP, 1500), form)
        signal, off, idx = ctx.ragged(list(x))
        wo, prob, mean, label = sc.run(signal, off, mode)
        ctx.finite("every window", prob)
        return {"prob": _take(prob, wo, idx), "mean": _take(mean, wo, idx), "label": _take(label, wo, idx), "windows": np.diff(wo)[idx]}


for _form in ("f32", "i16", "avg"):
    _scanner_case(_form)


def _scrubjay_scanner_case(form):
    name = "dsp_scrubjay_scanner_run_device" if form == "f32" else "dsp_scrubjay_scanner_run_pcm16_device"
    n = SCAN_CLIP if form == "f32" else 50001

    @case(f"C_scrubjay_scanner_run_{form}", name, "C", ELEM_OF_FORM[form], _ragged(n, ELEM_OF_FORM[form]),
          note="float samples on the 512-point front end, int16 on the 2048-point one of scrubjay_infer.c")
    def run(ctx, golden):
        from dsp_amd import scrubjay
        sj = _scrubjay(ctx, golden, "512" if form == "f32" else "2048")
        sc = ctx.once("sj_scanner", lambda: scrubjay.ScrubJayScanner(sj, window_frames=16, hop_frames=16))
        x, mode = as_input(probes_f32(n, 1600), form)
        signal, off, idx = ctx.ragged(list(x))
        wo, labels, dec, p1, feat = sc.run(signal, off, mode)
        ctx.finite("every window", feat)
        return {"labels": _take(labels, wo, idx), "decision": _take(dec, wo, idx), "prob1": _take(p1, wo, idx), "feat": _take(feat, wo, idx), "windows": np.diff(wo)[idx]}


for _form in ("f32", "i16", "avg"):
    _scrubjay_scanner_case(_form)


@case("C_stream_push", "dsp_stream_push_device", "C", "f32", _ragged(SCAN_CLIP, "f32"), note="one push; the fillers are streams of their own with a silent chunk of just under 2^31 samples")
def _(ctx, golden):
    import dsp_amd
    plan, stop, spk = _models(ctx, golden)
    signal, off, idx = ctx.ragged(list(probes_f32(SCAN_CLIP, 1700)))
    sess = dsp_amd.StreamSession(plan, off.size - 1, stop=stop, speaker=spk, window_frames=98, hop_frames=10)
    try:
        ro, rows, wo, prob, mean, label = sess.push(signal, off)
        ctx.torch.cuda.synchronize()
        ctx.finite("every window", prob)
        return {"rows": _take(rows, ro, idx), "prob": _take(prob, wo, idx), "mean": _take(mean, wo, idx), "label": _take(label, wo, idx),
                "new_rows": np.diff(ro)[idx], "new_windows": np.diff(wo)[idx]}
    finally:
        sess.close()


@case("C_stream_resample_push", "dsp_stream_resample_push_device", "C", "f32", _ragged(RESAMPLE_IN, "f32"),
      note="one push; the fillers are streams of their own with a silent chunk of just under 2^31 samples")
def _(ctx, golden):
    from dsp_amd import resample
    signal, off, idx = ctx.ragged(list(probes_f32(RESAMPLE_IN, 1800)))
    rs = resample.StreamResampler(44100, 16000, off.size - 1)
    try:
        out, oo = rs.push(signal, off)
        ctx.torch.cuda.synchronize()
        return {"out": _take(out, oo, idx), "lengths": np.diff(oo)[idx]}
    finally:
        rs.close()
