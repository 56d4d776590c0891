"""The resampler's kernel forms and tile geometries by name (dsp_amd/csrc/capi_resample.cpp make_shape, read through
dsp_resample_geometry): one ratio per class, the class pinned as literals, and the inputs of every name as functions of the name alone,
so that the CPU test that qualifies the references (tests/test_resample_shapes_cpu.py) and the GPU test that uses them
(tests/test_gpu_resample_shapes.py) see the same samples.

The forms: "staged_up1" resample_kernel<IN, true, true>, "staged" <IN, true, false>, "unstaged" <IN, false, false> (a branch too long
for the LDS budget: no live stream); the stream kernels are the twins of the two staged forms.  The copy (up = down = 1) has no geometry
to vary and stays with tests/test_gpu_resample.py.

THE TIGHT GATE.  The per-output bound of tests/test_gpu_resample.py, (L_k + 2) 2^-24 sum |h x|, is a worst case that grows with the
branch length: on 445 -> 1 (8901 taps) the float32 model sits at 0.0006 of it and a whole sidelobe tap set to zero at 0.035.  So a
recording of at least GATE_MIN_OUTPUTS outputs is also held to

    rms(got - ref64) <= MARGIN * rms(model32 - ref64)

where ref64 and model32 are resample_ref.resample in float64 and in float32 (products and sums rounded one by one, ascending input
sample: the kernel's order, whose FMA drops one of the two roundings per term).  Both sides are reference code.  The CPU test holds the
gate to mutants of the model on every name with more than 200 taps: each must fail it."""
import functools
import zlib

import numpy as np

from tests import resample_ref as R

# name -> (rate_in, rate_out, (form, tile, items, taps))
SHAPES = {
    "up1_down3": (48000, 16000, ("staged_up1", 2048, 512, 61)),
    "up1_down2": (16000, 8000, ("staged_up1", 3072, 768, 41)),
    "up1_down4": (64000, 16000, ("staged_up1", 2028, 507, 81)),           # the one up = 1 ratio whose second pass is not full
    "up1_down10": (160000, 16000, ("staged_up1", 908, 227, 201)),         # up = 1, less than one pass
    "up1_one_lane": (425, 1, ("staged_up1", 4, 1, 8501)),
    "up7_one_group": (1000, 7, ("staged", 28, 7, 2858)),
    "up64_half_pass": (1021, 64, ("staged", 512, 128, 320)),
    "cd_down": (44100, 16000, ("staged", 1920, 480, 56)),
    "cd_up": (16000, 44100, ("staged", 3528, 882, 21)),
    "up3": (16000, 48000, ("staged", 4092, 1023, 21)),
    "up1024": (1, 1024, ("staged", 4096, 1024, 21)),
    "near_unity_up": (1023, 1024, ("staged", 4096, 1024, 21)),
    "near_unity_down": (1024, 1023, ("staged", 4092, 1023, 21)),
    "unstaged_up1": (445, 1, ("unstaged", 1024, 256, 8901)),
    "unstaged_up3": (989, 3, ("unstaged", 1020, 255, 6594)),
    "unstaged_longest": (1024, 1, ("unstaged", 1024, 256, 20481)),
}
NAMES = list(SHAPES)
STAGED_NAMES = [n for n in NAMES if SHAPES[n][2][0] != "unstaged"]
LONG_NAMES = [n for n in NAMES if SHAPES[n][2][3] > 200]                   # the names whose mutants the tight gate must reject
INPUT_BUDGET = 1_000_000                                                   # input samples of one name's tile-edge recordings
BUDGETED = ("up1_one_lane", "unstaged_up1", "unstaged_up3")
FORMS = ("float", "mono", "stereo_ch0", "stereo_avg")
GATE_MIN_OUTPUTS = 64
MARGIN = 2.0


def form_of(geometry):
    """the kernel form launch_one picks for a geometry (dsp_amd.resample_geometry's dict)"""
    if geometry["up"] == 1 and geometry["down"] == 1:
        return "copy"
    if not geometry["staged"]:
        return "unstaged"
    return "staged_up1" if geometry["up"] == 1 else "staged"


def items_class(items):
    """how a block's work items fill its 256 lanes"""
    return "below_64" if items < 64 else "below_256" if items < 256 else "passes_full" if items % 256 == 0 else "last_pass_ragged"


def class_of(geometry):
    return form_of(geometry), geometry["tile"], geometry["items"], geometry["taps"]


def rates(name):
    return SHAPES[name][0], SHAPES[name][1]


def n_for_outputs(k, up, down):
    """the smallest n with ceil(n up / down) >= k (for up <= down: == k; an upsampler's output lengths skip values)"""
    return 0 if k <= 0 else ((k - 1) * down) // up + 1


def lengths(name):
    """The recording lengths of a name: no sample, 1 sample, 7 samples (shorter than any branch), and the smallest n whose output length
    reaches tile - 1, tile, tile + 1 and 2 tile + 3.  The BUDGETED names take those four in the order tile + 1, tile - 1, tile,
    2 tile + 3 for as long as the inputs stay within INPUT_BUDGET; unstaged_longest (20481 numpy steps per reference) takes output
    lengths 1, 3 and 5.  A name none of whose recordings reaches GATE_MIN_OUTPUTS outputs gets one of 67 outputs for the tight gate."""
    rate_in, rate_out = rates(name)
    up, down, _half = R.ratio(rate_in, rate_out)
    tile = SHAPES[name][2][1]
    if name == "unstaged_longest":
        targets = [1, 3, 5]
    elif name in BUDGETED:
        targets, total = [], 0
        for k in (tile + 1, tile - 1, tile, 2 * tile + 3):
            n = n_for_outputs(k, up, down)
            if total + n > INPUT_BUDGET:
                break
            targets.append(k)
            total += n
    else:
        targets = [tile - 1, tile, tile + 1, 2 * tile + 3]
    ns = [0, 1, 7] + [n_for_outputs(k, up, down) for k in targets]
    if max(R.out_len(n, up, down) for n in ns) < GATE_MIN_OUTPUTS:
        ns.append(n_for_outputs(67, up, down))
    return list(dict.fromkeys(ns))


def _rng(name, *salt):
    return np.random.default_rng([zlib.crc32(name.encode()), *salt])


def signal(rng, n, form):
    """uniform noise under a slow envelope in the caller's format -> (the recording, the float32 samples the kernels decode from it)"""
    env = np.repeat(rng.uniform(0.01, 1.0, n // 500 + 1), 500)[:n]
    if form == "float":
        x = (rng.uniform(-1, 1, n) * env).astype(np.float32)
        return x, x
    shape = (n,) if form == "mono" else (n, 2)
    pcm = np.clip(np.rint(rng.uniform(-32768, 32767, shape) * (env if form == "mono" else env[:, None])), -32768, 32767).astype(np.int16)
    return pcm, R.decode_pcm16(pcm, 1 if form == "stereo_avg" else 0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def recordings(name, form="float"):
    """-> ((raw, decoded float32), ...), one per lengths(name); read-only, computed once"""
    rng = _rng(name, FORMS.index(form))
    return tuple(_frozen(*signal(rng, n, form)) for n in lengths(name))


@functools.lru_cache(maxsize=None)
def references(name):
    """-> ((ref64, bound, model32 or None), ...) of recordings(name, "float"): the float64 definition, the per-output bound
    (L_k + 2) 2^-24 sum |h x|, and the float32 model where the tight gate applies"""
    rate_in, rate_out = rates(name)
    out = []
    for _raw, x in recordings(name):
        ref, mag, terms = R.resample(x, rate_in, rate_out, with_bound=True)
        model = R.resample(x, rate_in, rate_out, dtype=np.float32) if ref.size >= GATE_MIN_OUTPUTS else None
        out.append(_frozen(ref, (terms + 2) * 2.0 ** -24 * mag) + (None if model is None else _frozen(model)[0],))
    return tuple(out)


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def gate_ratio(got, ref64, model32):
    """rms(got - ref64) / rms(model32 - ref64): the tight gate passes at <= MARGIN"""
    assert got.shape == ref64.shape == model32.shape and ref64.size >= GATE_MIN_OUTPUTS
    floor = rms(model32.astype(np.float64) - ref64)
    assert floor > 0.0, "the float32 model has no rounding error on this recording: nothing to scale the gate by"
    return rms(np.asarray(got, np.float64) - ref64) / floor


def mutants(name, x):
    """The float32 model with one defect each, on the float32 samples x -> {what: y}.  Defects that are legitimately invisible are not
    here: the outermost taps are sin(10 pi) and a 2^-20 change of the centre tap is lost in rounding."""
    rate_in, rate_out = rates(name)
    up, down, half = R.ratio(rate_in, rate_out)
    h = R.taps(rate_in, rate_out)
    zeroed = h.copy()
    zeroed[half + int(8.5 * max(up, down))] = 0.0
    out = {"sidelobe_tap_zeroed": R.resample(x, rate_in, rate_out, dtype=np.float32, h64=zeroed),
           "one_sample_late": R.resample(np.concatenate([x[1:], np.zeros(1, x.dtype)]), rate_in, rate_out, dtype=np.float32)}
    if up > 1:
        out["next_branch"] = R.resample(x, rate_in, rate_out, dtype=np.float32, h64=np.concatenate([h[1:], [0.0]]))
    return out


def impulse_length(name):
    """samples of the impulse recording: the longest of lengths(name) -- more than one tile of outputs, and longer than a branch
    wherever a name has such a recording, so that most outputs see one impulse only"""
    return max(lengths(name))


@functools.lru_cache(maxsize=None)
def impulses(name):
    """A unit impulse at sample 0 and another at n - 1 -> (x float32, want float32, single, ref64, bound).  The output is the float32 taps
    themselves, want[k] = h[k down + half] + h[k down + half - (n - 1) up] with a tap outside [0, 2 half] counting as nothing: where
    `single` holds exactly one of the two is there and the kernel's sum is that tap, bit for bit (the other products are zeros); where
    both are there the sum of two goes under `bound` of ref64, the same sum of the float64 taps.  The taps are the library's own float64
    taps (dsp_resample_taps, host only), which the kernels' table is the float32 rounding of: at the sinc's zero crossings a tap is
    rounding noise of 1e-17, and the noise of resample_ref.taps is another (tests/test_resample_shapes_cpu.py holds the two sets to
    each other within the rounding gate of tests/test_resample_cpu.py)."""
    import dsp_amd
    rate_in, rate_out = rates(name)
    up, down, half = R.ratio(rate_in, rate_out)
    n = impulse_length(name)
    assert n >= 2
    x = np.zeros(n, np.float32)
    x[0] = x[n - 1] = 1.0
    h64 = dsp_amd.resample_taps(rate_in, rate_out)
    h32 = h64.astype(np.float32)
    k = np.arange(R.out_len(n, up, down), dtype=np.int64)
    want = np.zeros(k.size, np.float32)
    ref = np.zeros(k.size, np.float64)
    mag = np.zeros(k.size, np.float64)
    count = np.zeros(k.size, np.int64)
    for t in (k * down + half, k * down + half - (n - 1) * up):
        ok = (t >= 0) & (t <= 2 * half)
        want[ok] = want[ok] + h32[t[ok]]
        ref[ok] += h64[t[ok]]
        mag[ok] += np.abs(h64[t[ok]])
        count += ok
    return _frozen(x, want, count <= 1, ref, (count + 2) * 2.0 ** -24 * mag)


def stream_chunks(name):
    """the chunk lengths of a live feed at this ratio: T - 2, T - 1 (the carry's length), T, one sample, and the input of one tile of
    outputs less and plus one sample"""
    up, down, _half = R.ratio(*rates(name))
    _form, tile, _items, T = SHAPES[name][2]
    per_tile = down * tile // up
    return [T - 2, T - 1, T, 1, per_tile - 1, per_tile + 1]
