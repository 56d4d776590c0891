"""What every kind of MFCC plan answers to every use of a plan: the matrix tests/golden/make_golden_plan_uses.py records into
tests/golden/plan_uses.json and tests/test_gpu_plan_uses.py holds the library to.

A cell is one call on one plan: its return code, dsp_last_error() and, where the call was accepted, a SHA-256 over the bytes of its
outputs.  A refusal the Python layer makes before any C call is recorded by its exception text with rc None.  Scanners and stream
sessions are two cells each: the create call and the run / push on what it made.

Plans: every name of tests/mfcc512_shapes.py as created; the default plan under DSP_LOG_GLOBAL_REF1 and after
set_kernel(DSP_KERNEL_WAVE_FRAME); dsp_mfcc_speaker_config; a 1024-point plan as created, after set_kernel(DSP_KERNEL_ROW) and with a
prefilter; the 2048-point plan on the library's own semantics and on aubio's.

Inputs are the smallest that give every framing a frame, seeded noise: 2 clips of 3072 samples, a ragged pair of 3072 and 2500, 3
independent frames; the golden stop model; an SVM of 2 n_mfcc features with 3 support vectors drawn as test_gpu_scrubjay_scan.py's
_random_svm draws it.  int16 inputs are the noise at amplitude 20000, float inputs those samples / 32768."""
import hashlib
import os
import re

import numpy as np

from tests import mfcc512_shapes as M
from tests import signals as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "plan_uses.json")
CLIP, SHORT = 3072, 2500
WINDOW, HOP = 8, 4
FFT1024 = dict(n_fft=1024, frame_length=1024, hop_length=1024, n_mels=128)
DSP_EINVAL, DSP_EHIP = -1, -3


def _shape_plan(name):
    return lambda dsp: dsp.MfccPlan(M.config(name))


def _with_kernel(make, kernel):
    def build(dsp):
        plan = make(dsp)
        plan.set_kernel(kernel)
        return plan
    return build


def _cfg_plan(**over):
    return lambda dsp: dsp.MfccPlan(dsp.default_config(**over))


def _infer_config(**kw):
    from dsp_amd import scrubjay
    return scrubjay.scrubjay_infer_config(**kw)


PLANS = {f"shape:{name}": _shape_plan(name) for name in M.NAMES}
PLANS.update({
    "default_global_ref1": _cfg_plan(log_mode=1),
    "default_wave_frame": _with_kernel(_cfg_plan(), 2),
    "speaker400": lambda dsp: dsp.MfccPlan(dsp.speaker_config()),
    "fft1024": _cfg_plan(**FFT1024),
    "fft1024_row": _with_kernel(_cfg_plan(**FFT1024), 1),
    "fft1024_prefilter": _cfg_plan(prefilter=1, **FFT1024),
    "fft2048": lambda dsp: dsp.MfccPlan(_infer_config(aubio=False)),
    "fft2048_aubio": lambda dsp: dsp.MfccPlan(_infer_config()),
})
PLAN_NAMES = list(PLANS)

USES = ["frames", "clips", "clips_pcm16", "ragged", "ragged_pcm16", "label", "label_pcm16", "label_ragged", "label_ragged_pcm16", "stop",
        "stop_pcm16", "stop_ragged", "stop_ragged_pcm16", "scanner_create", "scanner_run_pcm16", "scrubjay_scanner_create",
        "scrubjay_scanner_run_pcm16", "stream_create", "stream_push", "stream_pcm16_create", "stream_pcm16_push"]


def _pcm(n, seed):
    return np.round(S.uniform_pm1(n, seed) * np.float32(20000.0)).astype(np.int16)


def inputs():
    """host arrays, the same for every plan (the frames entry takes its frame length from the plan)"""
    clips = np.stack([_pcm(CLIP, 11), _pcm(CLIP, 12)])
    ragged = np.concatenate([_pcm(CLIP, 13), _pcm(SHORT, 14)])
    return {"clips": clips, "ragged": ragged, "offsets": np.array([0, CLIP, CLIP + SHORT], np.int64)}


def random_svm(rng, n_sv, n_coef):
    nf = 2 * n_coef
    return {"offset": rng.normal(0, 3, nf).astype(np.float32), "scale": rng.uniform(0.05, 0.5, nf).astype(np.float32),
            "sv": rng.normal(0, 1, (n_sv, nf)).astype(np.float32), "coef": rng.normal(0, 1, n_sv).astype(np.float32),
            "kernel_params": np.array([1.0 / nf, 0.0, 3.0], np.float32), "rho": np.array([rng.normal(0, 0.5)], np.float32),
            "prob_a": np.array([-rng.uniform(0.5, 3)], np.float32), "prob_b": np.array([rng.normal(0, 0.3)], np.float32)}


def _digest(torch, outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for o in outs if isinstance(outs, (tuple, list)) else (outs,):
        if o is None:
            continue
        a = o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o)
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cell(torch, call):
    """-> (the cell, what the call returned or None)"""
    from dsp_amd import lib as dl
    try:
        out = call()
    except dl.DspError as e:
        m = re.fullmatch(r"\S+ failed \((-?\d+)\): (.*)", str(e), re.S)
        if not m:
            return {"rc": None, "error": f"DspError: {e}"}, None
        return {"rc": int(m.group(1)), "error": m.group(2)}, None
    except (ValueError, TypeError, AssertionError) as e:
        return {"rc": None, "error": f"{type(e).__name__}: {e}"}, None
    return {"rc": 0, "error": "", "sha256": _digest(torch, out) if not hasattr(out, "close") else None}, out


def run_plan(torch, name, stop_params):
    """every use on plan `name` -> {use: cell}"""
    import dsp_amd
    from dsp_amd import scrubjay
    x = inputs()
    plan = PLANS[name](dsp_amd)
    cfg = plan.cfg
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    as_float = lambda a: (a.astype(np.float32) / np.float32(32768.0))      # noqa: E731
    clips_i, ragged_i = dev(x["clips"]), dev(x["ragged"])
    clips_f, ragged_f = dev(as_float(x["clips"])), dev(as_float(x["ragged"]))
    frames = dev(as_float(_pcm(3 * cfg.frame_length, 15)).reshape(3, cfg.frame_length))
    off = x["offsets"]
    big = 1 << 20
    sj = scrubjay.ScrubJay.__new__(scrubjay.ScrubJay)
    sj.plan, sj.svm = plan, scrubjay.SvmModel(random_svm(np.random.default_rng(PLAN_NAMES.index(name)), 3, cfg.n_mfcc))
    stop = dsp_amd.StopModel(stop_params)
    cells = {}

    def put(use, call):
        cells[use], out = cell(torch, call)
        return out

    put("frames", lambda: plan.frames(frames))
    put("clips", lambda: plan.clips(clips_f, big))
    put("clips_pcm16", lambda: plan.clips_pcm16(clips_i, big))
    put("ragged", lambda: plan.clips_ragged(ragged_f, off, big))
    put("ragged_pcm16", lambda: plan.clips_ragged(ragged_i, off, big))
    put("label", lambda: sj(clips_f))
    put("label_pcm16", lambda: sj.pcm16(clips_i))
    put("label_ragged", lambda: sj.ragged(ragged_f, off))
    put("label_ragged_pcm16", lambda: sj.ragged(ragged_i, off))
    put("stop", lambda: stop.classify_signal_batch(plan, clips_f))
    put("stop_pcm16", lambda: stop.classify_signal_batch_pcm16(plan, clips_i))
    put("stop_ragged", lambda: stop.classify_signal_ragged(plan, ragged_f, off))
    put("stop_ragged_pcm16", lambda: stop.classify_signal_ragged(plan, ragged_i, off))
    made = []
    for create, run, make, use in (
            ("scanner_create", "scanner_run_pcm16", lambda: dsp_amd.Scanner(plan, stop=stop, window_frames=WINDOW, hop_frames=HOP),
             lambda s: s.run(ragged_i, off)),
            ("scrubjay_scanner_create", "scrubjay_scanner_run_pcm16", lambda: scrubjay.ScrubJayScanner(sj, WINDOW, HOP), lambda s: s.run(ragged_i, off)),
            ("stream_create", "stream_push", lambda: dsp_amd.StreamSession(plan, 2), lambda s: s.push(ragged_f, off)),
            ("stream_pcm16_create", "stream_pcm16_push", lambda: dsp_amd.StreamSession(plan, 2, dtype=torch.int16), lambda s: s.push(ragged_i, off))):
        obj = put(create, make)
        if obj is None:
            cells[run] = {"rc": None, "error": "not created"}
        else:
            made.append(obj)
            put(run, lambda: use(obj))
    torch.cuda.synchronize()
    for obj in made:
        obj.close()
    for obj in (stop, sj.svm, plan):
        obj.close()
    assert list(cells) == USES
    return cells
