"""Stream order of the device entry points (include/dsp_amd.h: "work is enqueued on `stream` ... and the call returns without
synchronising"): the harness and the table of cases that tests/test_gpu_stream_order.py runs on a GPU and that
tests/test_stream_order_cpu.py holds against the header without one.

A case is a small call, or a chain of calls on carried state, of one family of entries.  The harness runs it in three ways:

  quiet   on torch's default stream, the device synchronised before and after: once to warm up (lazy kernel loading, tables,
          workspaces), once for the reference, and once more for t_host, the host's time for the call and the device's work behind it;
  decoy   the same on other valid inputs (every float input scaled by 0.75), so that no workspace, table or accumulator of a handle
          still holds what the reference run left there: a step that reads stale state would otherwise read the right values;
  late    on a NON-BLOCKING side stream, behind a delay kernel: the inputs are poison (NaN, or 0 for integers and flags) until copies
          enqueued behind the delay fill them in, the outputs are sentinel bytes with spare entries behind them, and a copy of every
          output (the caller's consumer) is enqueued behind the calls.  The host waits for nothing until all of it is enqueued.

Asserted: the consumer's copies equal the quiet run's bit for bit, spare entries included; every C name the case declares was reached;
and for every entry that is not documented to wait, the event recorded behind the delay had NOT completed when the C function
returned (read through a tap on the ctypes function itself, so that a Python wrapper's own work does not count).  Within a chain the
event is asserted up to the first entry that waits: behind a wait the stream is drained and the event says nothing.

The delay is 100 ms, or 10 t_host where that is more, 1 s at most; a case that cannot meet 10 t_host within 1 s is too big.

Outputs are allocated by the library's own Python layer with torch.empty or torch.zeros; while a case runs the harness stands in for
both on CUDA devices, hands out views of larger buffers filled with SENTINEL bytes (zeroed in front, for torch.zeros) and keeps the
buffers, which is how the spare entries get behind outputs the wrappers size themselves.  (empty_like and zeros_like are left alone:
such outputs are compared, without spares.)

A ring of upload slots (dsp_amd/csrc/capi_util.hpp SpanRing) carries host tables to the device.  It used to have four slots and an
acquirer waited for the event of the slot before it: the fifth lease enqueued behind an unfinished producer blocked the host, which
dsp_time_stretch_ragged_device (three leases) and dsp_augment_ragged_device (four) hit in the chain below.  The ring now grows."""
import ctypes as C
import dataclasses
import gc
import os
import time

import numpy as np

SENTINEL = 0x5A              # every byte of an output before the call (as float32: 1.5e16, finite; as int32: 1515870810)
SPARE = 64                   # entries behind every captured output
DELAY_MS, DELAY_MAX_MS, DELAY_FACTOR = 100.0, 1000.0, 10.0
DECOY_SCALE = 0.75

# entries that cannot run on one GPU without RCCL would be named here with the reason; the header declares none (dsp_gather_* has no
# *_device name)
EXEMPT = {}


@dataclasses.dataclass
class Case:
    id: str
    names: tuple                 # the C entry points the case reaches, in the order of its first calls
    build: object                # build(golden) -> (state, inputs): inputs a dict of numpy arrays that go to the device
    run: object                  # run(state, dev) -> dict of outputs (CUDA tensors, numpy arrays or None), dev the inputs on the device
    waits: tuple = ()            # those of `names` that the header documents to wait for the stream
    reset: object = None         # reset(state): forget carried state between runs (stream sessions)
    env: dict = None             # environment variables that select a launch chain, set while the case runs
    note: str = ""


CASES = []


def case(id, names, waits=(), reset=None, env=None, note=""):
    """decorator of a build function that returns (state, inputs, run)"""
    names = (names,) if isinstance(names, str) else tuple(names)
    waits = (waits,) if isinstance(waits, str) else tuple(waits)

    def register(build):
        def split(golden):
            state, inputs, run = build(golden)
            return (state, run), inputs
        CASES.append(Case(id, names, split, lambda st, dev: st[1](st[0], dev), waits, (lambda st: reset(st[0])) if reset else None, env, note))
        return build
    return register


# ---- the harness --------------------------------------------------------------------------------------------------------------------

_session = {}


def hip_runtime():
    """the HIP runtime already loaded in this process (torch's), through ctypes"""
    if "hip" not in _session:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "no HIP runtime is loaded in this process"
        _session["hip"] = C.CDLL(path)
    return _session["hip"]


def side_stream(torch):
    """one non-blocking stream per session: a pool stream of torch's if hipStreamGetFlags says it is one, else our own"""
    if "stream" not in _session:
        hip = hip_runtime()
        hip.hipStreamGetFlags.argtypes, hip.hipStreamGetFlags.restype = [C.c_void_p, C.POINTER(C.c_uint)], C.c_int
        s, flags = torch.cuda.Stream(), C.c_uint(0)
        assert hip.hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(flags)) == 0
        if not flags.value & 1:                                  # hipStreamNonBlocking
            raw = C.c_void_p()
            hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamCreateWithFlags.restype = [C.POINTER(C.c_void_p), C.c_uint], C.c_int
            assert hip.hipStreamCreateWithFlags(C.byref(raw), 1) == 0
            s = torch.cuda.ExternalStream(raw.value)
            assert hip.hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(flags)) == 0
        assert flags.value & 1, "the side stream is not non-blocking"
        _session["stream"] = s
    return _session["stream"]


def cycles_per_ms(torch):
    """torch.cuda._sleep's cycles per millisecond, measured once per session with two events (printed, never asserted)"""
    if "cpm" not in _session:
        n = 20_000_000
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        torch.cuda.synchronize()
        _session["cpm"] = n / max(a.elapsed_time(b), 1e-3)
        print(f"stream order: torch.cuda._sleep runs {_session['cpm']:.0f} cycles per ms")
    return _session["cpm"]


class Outputs:
    """stands in for torch.empty and torch.zeros on CUDA devices while a case runs (see the module's docstring)"""

    def __init__(self, torch):
        self.torch, self.real, self.real_zeros, self.buffers = torch, torch.empty, torch.zeros, []

    def _make(self, real, zero, size, dtype, device, kw):
        torch = self.torch
        if device is None or torch.device(device).type != "cuda" or kw:
            return real(*size, dtype=dtype, device=device, **kw)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(int(v) for v in size)
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        full = self.real(n + SPARE, dtype=dtype, device=device)
        full.view(torch.uint8).fill_(SENTINEL)
        if zero:
            full[:n].zero_()
        self.buffers.append((full, n))
        return full[:n].view(shape)

    def empty(self, *size, dtype=None, device=None, **kw):
        return self._make(self.real, False, size, dtype, device, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        return self._make(self.real_zeros, True, size, dtype, device, kw)

    def __enter__(self):
        self.torch.empty, self.torch.zeros = self.empty, self.zeros
        return self

    def __exit__(self, *exc):
        self.torch.empty, self.torch.zeros = self.real, self.real_zeros


class Tap:
    """wraps the ctypes functions `names` of the loaded library: after each call, which name it was, whether `gate` had completed by
    then and how long the host was inside"""

    def __init__(self, lib, names, gate):
        self.lib, self.names, self.gate, self.calls, self.saved = lib, names, gate, [], {}

    def __enter__(self):
        for name in self.names:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def tapped(*args, _fn=fn, _name=name):
                t0 = time.perf_counter()
                rc = _fn(*args)
                passed = self.gate.query() if self.gate is not None else None
                self.calls.append((_name, passed, time.perf_counter() - t0))
                return rc
            setattr(self.lib, name, tapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def _bytes(x):
    """an output on the host as bytes: CUDA tensor, numpy array, number, or a list / tuple / dict of them"""
    if x is None:
        return b""
    if isinstance(x, dict):
        return b"".join(_bytes(x[k]) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return b"".join(_bytes(v) for v in x)
    if hasattr(x, "is_cuda"):
        x = x.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(x).tobytes()


def _clone(x):
    """the consumer's copy of an output, enqueued on the current stream (host values are copied as they are)"""
    if x is None:
        return None
    if isinstance(x, dict):
        return {k: _clone(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clone(v) for v in x]
    if hasattr(x, "is_cuda"):
        return x.clone()
    return np.array(x, copy=True)


def _poison(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.fill_(float("nan")) if t.is_floating_point() else t.zero_()


def _decoy(a):
    return (a * a.dtype.type(DECOY_SCALE)).astype(a.dtype) if a.dtype.kind == "f" else a


def _once(torch, c, state, dev, lib, gate=None):
    """the case's calls and the consumer's copies, enqueued on the current stream -> (copies of the named outputs, copies of the
    captured buffers with their sizes, the tapped calls)"""
    with Outputs(torch) as outs, Tap(lib, c.names, gate) as tap:
        named = c.run(state, dev)
    return _clone(named), [(full.clone(), n) for full, n in outs.buffers], tap.calls


def run_case(torch, c, golden):
    """-> the report line of the case (a dict); asserts what the module's docstring states"""
    import dsp_amd.lib as dl
    lib = dl.load()
    old_env = {k: os.environ.get(k) for k in (c.env or {})}
    os.environ.update(c.env or {})
    try:
        state, host = c.build(golden)
        host = {k: np.ascontiguousarray(v) for k, v in host.items()}
        quiet_in = {k: torch.from_numpy(v).cuda() for k, v in host.items()}

        def quiet(dev):
            if c.reset:
                c.reset(state)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = _once(torch, c, state, dev, lib)
            torch.cuda.synchronize()
            return got, time.perf_counter() - t0

        quiet(quiet_in)               # warms lazy kernel loading, tables, workspaces and LDS-limit attributes: the runs behind it allocate alike
        (ref_named, ref_bufs, ref_calls), _ = quiet(quiet_in)
        ref_named, ref_bufs = _bytes(ref_named), [(_bytes(full), n) for full, n in ref_bufs]
        reached = {name for name, _, _ in ref_calls}
        assert reached == set(c.names), f"{c.id}: declares {sorted(c.names)}, reaches {sorted(reached)}"
        _, t_host = quiet(quiet_in)
        quiet({k: torch.from_numpy(_decoy(v)).cuda() for k, v in host.items()})

        delay_ms = min(max(DELAY_MS, DELAY_FACTOR * t_host * 1e3), DELAY_MAX_MS)
        assert delay_ms >= DELAY_FACTOR * t_host * 1e3, f"{c.id}: t_host {t_host * 1e3:.1f} ms is too long for a delay of {DELAY_MAX_MS:.0f} ms: shrink the case"
        cycles = int(delay_ms * cycles_per_ms(torch))
        late_in = {k: _poison(torch, v) for k, v in host.items()}
        if c.reset:
            c.reset(state)
        s, gate = side_stream(torch), torch.cuda.Event()
        # no collection of cyclic garbage while the host must not wait: a handle of an earlier test that is collected now is destroyed
        # now, and a destroy function frees device memory, which waits for the whole device -- the delay included
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
                gate.record(s)
                for k in late_in:
                    late_in[k].copy_(quiet_in[k], non_blocking=True)
                named, bufs, calls = _once(torch, c, state, late_in, lib, gate)
            still_behind = not gate.query()
            s.synchronize()
        finally:
            if collecting:
                gc.enable()

        assert {name for name, _, _ in calls} == set(c.names), c.id
        asserted, early = 0, []
        for name, passed, _ in calls:
            if name in c.waits:
                break
            asserted += 1
            if passed:
                early.append(name)
        assert not early, f"{c.id}: the delay had ended when {early} returned: the call waited for the stream"
        assert _bytes(named) == ref_named, f"{c.id}: an output differs from the quiet run"
        assert len(bufs) == len(ref_bufs), c.id
        for i, ((full, n), (ref, ref_n)) in enumerate(zip(bufs, ref_bufs)):
            assert n == ref_n, (c.id, i)
            got = _bytes(full)
            item = len(got) // (n + SPARE)
            assert got[n * item:] == bytes([SENTINEL]) * (SPARE * item), f"{c.id}: output {i}: the spare entries were written"
            assert got == ref, f"{c.id}: output {i} differs from the quiet run"
        return {"case": c.id, "t_host_ms": round(t_host * 1e3, 3), "delay_ms": round(delay_ms, 1), "calls": len(calls),
                "returned_before_gate": [name for name, passed, _ in calls if not passed], "gate_asserted_on": asserted,
                "enqueued_before_gate": still_behind, "outputs": len(bufs), "waits": list(c.waits),
                "host_ms_in_calls": round(sum(t for _, _, t in calls) * 1e3, 3)}
    finally:
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def line(r):
    return (f"{r['case']:<44} t_host {r['t_host_ms']:8.3f} ms  delay {r['delay_ms']:6.1f} ms  calls {r['calls']:2d}  before the gate "
            f"{len(r['returned_before_gate']):2d} (asserted on {r['gate_asserted_on']:2d})  outputs {r['outputs']:2d}  host in calls "
            f"{r['host_ms_in_calls']:8.3f} ms  consumer enqueued before the gate: {'yes' if r['enqueued_before_gate'] else 'no '}  "
            f"waits: {', '.join(r['waits']) or '-'}")


def covered():
    """every C name a case declares -> the ids of its cases"""
    out = {}
    for c in CASES:
        for name in c.names:
            out.setdefault(name, []).append(c.id)
    return out


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------

def _S():
    from tests import signals
    return signals


def noise(n, seed, level=0.5):
    return (_S().uniform_pm1(int(n), seed) * np.float32(level)).astype(np.float32)


def pcm16(x):
    return np.round(np.asarray(x, np.float64) * 32767.0).astype(np.int16)


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


CLIP = 6129                                    # samples of an MFCC clip: no multiple of a hop, 36 rows of 400 / 160


def strided(x):
    """[n][odd] -> [n][odd + 1], one spare sample behind every clip: the clip entries take an even clip stride; cases pass the view
    dev[...][:, :odd]"""
    return np.ascontiguousarray(np.concatenate([x, np.zeros_like(x[:, :1])], axis=1))
RAGGED = (6129, 399, 4000, 0, 2049)            # a clip below a frame and one without samples among the others


def _models(golden):
    """(MfccPlan of the default config, StopModel, SpeakerModel) of the golden parameters"""
    import dsp_amd
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return dsp_amd.MfccPlan(dsp_amd.default_config()), dsp_amd.StopModel(dict(golden("stop_model.npz"))), dsp_amd.SpeakerModel(t, u)


def _svm_attrs(golden):
    m = golden("scrubjay_svm.npz")
    return {k: m[k] for k in m.files}


# ---- MFCC: frames, clips, ragged; 512, 2048, 400, the 1024 prefilter plan; int16 ----------------------------------------------------------

def _mfcc_cfg(kind, log_mode):
    import dsp_amd
    from dsp_amd import scrubjay
    if kind == "512":
        return dsp_amd.default_config(log_mode=log_mode)
    if kind == "2048":
        cfg = scrubjay.scrubjay_infer_config(aubio=False)
        cfg.log_mode = log_mode
        return cfg
    if kind == "aubio2048":
        return scrubjay.scrubjay_infer_config()
    if kind == "400":
        return dsp_amd.speaker_config(log_mode=log_mode)
    assert kind == "1024prefilter"
    return dsp_amd.default_config(prefilter=2, n_fft=1024, frame_length=1024, hop_length=1024, n_mels=128)


def _mfcc_case(form, kind, log_mode, env=None, tag=""):
    name = {"frames": "dsp_mfcc_frames_device", "clips": "dsp_mfcc_clips_device", "ragged": "dsp_mfcc_clips_ragged_device",
            "clips_pcm16": "dsp_mfcc_clips_pcm16_device", "ragged_pcm16": "dsp_mfcc_clips_ragged_pcm16_device"}[form]

    @case(f"mfcc_{form}_{kind}_log{log_mode}{tag}", name, env=env)
    def build(golden):
        import dsp_amd
        cfg = _mfcc_cfg(kind, log_mode)
        plan = dsp_amd.MfccPlan(cfg)
        fl = cfg.frame_length
        if form == "frames":
            x = noise(37 * fl, 11).reshape(37, fl)
            x[5] = 0.0
            x[6] *= np.float32(1e-3)
            return plan, {"x": x}, lambda plan, dev: {"mfcc": plan.frames(dev["x"])}
        if form.startswith("clips"):
            x = noise(4 * CLIP, 12).reshape(4, CLIP)
            x[1, 2000:] *= np.float32(1e-3)
            x[2, :3000] = 0.0
            if form == "clips":
                return plan, {"x": strided(x)}, lambda plan, dev: {"mfcc": plan.clips(dev["x"][:, :CLIP], 1 << 20)}
            return plan, {"x": strided(pcm16(x))}, lambda plan, dev: {"mfcc": plan.clips_pcm16(dev["x"][:, :CLIP], 1 << 20)}
        off = offsets_of(RAGGED)
        x = noise(off[-1], 13)
        x[100:3000] *= np.float32(1e-3)
        if form == "ragged_pcm16":
            x = pcm16(x)
        return plan, {"x": x}, lambda plan, dev: {"mfcc": plan.clips_ragged(dev["x"], off, 1 << 20)[0]}


for _kind in ("512", "2048", "400"):
    for _form in ("frames", "clips", "ragged"):
        for _log in (0, 1):
            _mfcc_case(_form, _kind, _log)
_mfcc_case("frames", "1024prefilter", 0)
_mfcc_case("frames", "1024prefilter", 0, env={"DSP_AMD_PREFILTER_TWO_PASS": "1"}, tag="_two_pass")
for _kind, _log in (("512", 0), ("aubio2048", 2)):
    _mfcc_case("clips_pcm16", _kind, _log)
    _mfcc_case("ragged_pcm16", _kind, _log)


# ---- the fused kernels: scrub-jay label, classify_signal ----------------------------------------------------------------------------

def _scrubjay(golden, kind):
    from dsp_amd import scrubjay
    return scrubjay.ScrubJay(_svm_attrs(golden), config=None if kind == "512" else scrubjay.scrubjay_infer_config())


def _fused_outputs(out):
    return dict(zip(("labels", "decision", "prob1", "feat"), out))


def _scrubjay_case(kind, form):
    name = {"float": "dsp_scrubjay_fused_device", "pcm16": "dsp_scrubjay_fused_pcm16_device", "ragged": "dsp_scrubjay_fused_ragged_device",
            "ragged_pcm16": "dsp_scrubjay_fused_ragged_pcm16_device"}[form]

    @case(f"scrubjay_fused_{kind}_{form}", name)
    def build(golden):
        sj = _scrubjay(golden, kind)
        if form in ("float", "pcm16"):
            x = noise(4 * CLIP, 21).reshape(4, CLIP)
            x[3] = _S().chirp(CLIP, 300.0, 6000.0)
            if form == "float":
                return sj, {"x": strided(x)}, lambda sj, dev: _fused_outputs(sj(dev["x"][:, :CLIP]))
            return sj, {"x": strided(pcm16(x))}, lambda sj, dev: _fused_outputs(sj.pcm16(dev["x"][:, :CLIP]))
        lens = (6129, 4000, 2049, 9001)
        off = offsets_of(lens)
        x = noise(off[-1], 22)
        if form == "ragged_pcm16":
            x = pcm16(x)
        return sj, {"x": x}, lambda sj, dev: _fused_outputs(sj.ragged(dev["x"], off))


for _kind in ("512", "2048"):
    for _form in ("float", "pcm16", "ragged", "ragged_pcm16"):
        _scrubjay_case(_kind, _form)


def _signal_case(form, env=None, tag=""):
    name = {"float": "dsp_classify_signal_batch_device", "pcm16": "dsp_classify_signal_batch_pcm16_device",
            "ragged": "dsp_classify_signal_batch_ragged_device", "ragged_pcm16": "dsp_classify_signal_batch_ragged_pcm16_device"}[form]

    @case(f"classify_signal_{form}{tag}", name, env=env)
    def build(golden):
        plan, stop, _spk = _models(golden)
        if form in ("float", "pcm16"):
            x = noise(4 * 16000, 31).reshape(4, 16000)
            x[1, 8000:] *= np.float32(1e-3)
            if form == "float":
                return (plan, stop), {"x": x}, lambda st, dev: {"prob": st[1].classify_signal_batch(st[0], dev["x"])}
            return (plan, stop), {"x": pcm16(x)}, lambda st, dev: {"prob": st[1].classify_signal_batch_pcm16(st[0], dev["x"])}
        off = offsets_of((16000, 400, 9000, 20001))          # (a clip of exactly one frame)
        x = noise(off[-1], 32)
        if form == "ragged_pcm16":
            x = pcm16(x)
        return (plan, stop), {"x": x}, lambda st, dev: {"prob": st[1].classify_signal_ragged(st[0], dev["x"], off)}


for _form in ("float", "pcm16", "ragged", "ragged_pcm16"):
    _signal_case(_form)
_signal_case("float", env={"DSP_AMD_STOP_TWO_KERNELS": "1"}, tag="_two_kernels")


# ---- the classifiers: float32 and float64, _cfg, pcm16, ragged ------------------------------------------------------------------------

def _classify_clips():
    """clips with midpoints (bursts) and without (noise, silence): the gated second spectrogram and the float64 undecided-segment
    list run, and are skipped, in one batch"""
    c = _S().classify_cases()
    return np.stack([c[k] for k in ("noise", "burst_2k", "jay_like", "scrub_a", "silence")])


CLASSIFY_RAGGED = (16000, 14000, 16000, 15000, 8000)


def _classify_case(f64, form):
    suffix = "_f64" if f64 else ""
    name = {"plain": "dsp_classify_batch_device", "cfg": "dsp_classify_batch_device_cfg", "pcm16": "dsp_classify_batch_pcm16_device",
            "ragged": "dsp_classify_batch_ragged_device", "ragged_pcm16": "dsp_classify_batch_ragged_pcm16_device"}[form]
    if f64 and form == "cfg":
        return
    cname = name + suffix

    @case(f"classify{suffix or '_f32'}_{form}", cname)
    def build(golden):
        import importlib
        K = importlib.import_module("dsp_amd.classify")      # (dsp_amd.classify, the name, is the reference's function)
        clips = _classify_clips()
        dtype = np.float64 if f64 else np.float32
        if form == "plain" and not f64:
            def run(_, dev):
                import torch
                import dsp_amd.lib as dl
                x = dev["x"]
                labels = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
                dl.check(dl.load().dsp_classify_batch_device(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), labels.data_ptr(), dl.current_stream(x)),
                         "dsp_classify_batch_device")
                return {"labels": labels}
            return None, {"x": clips}, run
        if form == "plain":
            return None, {"x": clips.astype(dtype)}, lambda _, dev: {"labels": K.classify_device_f64(dev["x"], config=K.CLASSIFY_DONUT_C)}
        if form == "cfg":
            return None, {"x": clips}, lambda _, dev: {"labels": K.classify_device(dev["x"], config=K.CLASSIFY_MICROPHONE)}
        if form == "pcm16":
            fn = K.classify_device_f64_pcm16 if f64 else K.classify_device_pcm16
            return None, {"x": pcm16(clips)}, lambda _, dev: {"labels": fn(dev["x"])}
        off = offsets_of(CLASSIFY_RAGGED)
        x = np.concatenate([c[:n] for c, n in zip(clips, CLASSIFY_RAGGED)])
        x = pcm16(x) if form == "ragged_pcm16" else x.astype(dtype)
        fn = K.classify_device_ragged_f64 if f64 else K.classify_device_ragged
        return None, {"x": x}, lambda _, dev: {"labels": fn(dev["x"], off)}


for _f64 in (False, True):
    for _form in ("plain", "cfg", "pcm16", "ragged", "ragged_pcm16"):
        _classify_case(_f64, _form)


# ---- the consumers of an MFCC matrix ----------------------------------------------------------------------------------------------------

def _rows(n, d, seed, scale=8.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(np.float32)


SCAN_FO = offsets_of((150, 97, 230))            # a recording below a window (98 rows) between two above it


@case("stop_predict", "dsp_stop_predict_device")
def _(golden):
    _plan, stop, _spk = _models(golden)
    x = _rows(5 * 98, 13, 41).reshape(5, 98, 13)
    return stop, {"x": x}, lambda stop, dev: {"prob": stop.predict(dev["x"])}


@case("speaker_llr", "dsp_speaker_llr_device")
def _(golden):
    _plan, _stop, spk = _models(golden)
    x = _rows(5 * 37, spk.d, 42, 3.0).reshape(5, 37, spk.d)
    return spk, {"x": x}, lambda spk, dev: dict(zip(("mean", "label", "ll_target", "ll_ubm"), spk.llr(dev["x"], per_frame=True)))


@case("speaker_llr_ragged", "dsp_speaker_llr_ragged_device")
def _(golden):
    _plan, _stop, spk = _models(golden)
    fo = offsets_of((1, 37, 64, 65, 300))
    x = _rows(fo[-1], spk.d, 43, 3.0)
    return spk, {"x": x}, lambda spk, dev: dict(zip(("mean", "label", "ll_target", "ll_ubm"), spk.llr_ragged(dev["x"], fo, per_frame=True)))


@case("stop_scan", "dsp_stop_scan_device")
def _(golden):
    _plan, stop, _spk = _models(golden)
    x = _rows(SCAN_FO[-1], 13, 44)
    return stop, {"x": x}, lambda stop, dev: {"prob": stop.scan(dev["x"], SCAN_FO, 98, 10)[1]}


@case("speaker_scan", "dsp_speaker_scan_device")
def _(golden):
    _plan, _stop, spk = _models(golden)
    x = _rows(SCAN_FO[-1], spk.d, 45, 3.0)
    return spk, {"x": x}, lambda spk, dev: dict(zip(("mean", "label"), spk.scan(dev["x"], SCAN_FO, 98, 10)[1:]))


def _scanner_case(pcm):
    @case("scanner_run" + ("_pcm16" if pcm else ""), "dsp_scanner_run_pcm16_device" if pcm else "dsp_scanner_run_device")
    def build(golden):
        import dsp_amd
        plan, stop, spk = _models(golden)
        sc = dsp_amd.Scanner(plan, stop=stop, speaker=spk, window_frames=98, hop_frames=10)
        off = offsets_of((24000, 400, 15920, 30001))         # one frame; exactly 98 rows
        x = noise(off[-1], 46)
        return sc, {"x": pcm16(x) if pcm else x}, lambda sc, dev: dict(zip(("prob", "mean", "label"), sc.run(dev["x"], off)[1:]))


_scanner_case(False)
_scanner_case(True)


@case("svm_predict", "dsp_svm_predict_device")
def _(golden):
    from dsp_amd import scrubjay
    m = golden("scrubjay_svm.npz")
    svm = scrubjay.SvmModel(_svm_attrs(golden))
    x = np.stack([(m["offset"] + _S().uniform_pm1(40, 900 + i) * (2.5 / m["scale"])).astype(np.float32) for i in range(65)])
    return svm, {"x": x}, lambda svm, dev: dict(zip(("labels", "decision", "prob1"), svm.predict(dev["x"])))


@case("svm_scan", "dsp_svm_scan_device")
def _(golden):
    from dsp_amd import scrubjay
    svm = scrubjay.SvmModel(_svm_attrs(golden))
    fo = offsets_of((40, 15, 77))
    x = _rows(fo[-1], 20, 47)
    return svm, {"x": x}, lambda svm, dev: dict(zip(("labels", "decision", "prob1", "feat"), svm.scan(dev["x"], fo, 16, 4)[1:]))


def _scrubjay_scanner_case(pcm):
    @case("scrubjay_scanner_run" + ("_pcm16" if pcm else ""), "dsp_scrubjay_scanner_run_pcm16_device" if pcm else "dsp_scrubjay_scanner_run_device")
    def build(golden):
        from dsp_amd import scrubjay
        sj = _scrubjay(golden, "2048" if pcm else "512")      # (int16 scans run on the scrubjay_infer.c front end)
        sc = scrubjay.ScrubJayScanner(sj, window_frames=16, hop_frames=4)
        off = offsets_of((30000, 2048, 16384, 50001) if pcm else (9000, 400, 2800, 12001))
        x = noise(off[-1], 48)
        return sc, {"x": pcm16(x) if pcm else x}, lambda sc, dev: dict(zip(("labels", "decision", "prob1", "feat"), sc.run(dev["x"], off)[1:]))


_scrubjay_scanner_case(False)
_scrubjay_scanner_case(True)


@case("mfcc_stats", "dsp_mfcc_stats_device")
def _(golden):
    from dsp_amd import scrubjay
    x = _rows(5 * 37, 20, 49).reshape(5, 37, 20)
    return None, {"x": x}, lambda _, dev: {"feat": scrubjay.mfcc_stats(dev["x"])}


@case("upsample_linear", "dsp_upsample_linear_device")
def _(golden):
    import dsp_amd
    x = noise(4 * 1000, 50).reshape(4, 1000)
    return None, {"x": x}, lambda _, dev: {"out": dsp_amd.upsample_linear(dev["x"], 2205)}


# ---- the resampler ------------------------------------------------------------------------------------------------------------------------

def _resample_case(form):
    name = {"clips": "dsp_resample_clips_device", "clips_pcm16": "dsp_resample_clips_pcm16_device", "ragged": "dsp_resample_ragged_device",
            "ragged_pcm16": "dsp_resample_ragged_pcm16_device"}[form]

    @case(f"resample_{form}", name)
    def build(golden):
        from dsp_amd import resample
        rs = resample.Resampler(44100, 16000)
        if form.startswith("clips"):
            x = noise(3 * 4411, 51).reshape(3, 4411)
            if form == "clips":
                return rs, {"x": x}, lambda rs, dev: {"out": rs.clips(dev["x"])}
            st = np.stack([pcm16(x), pcm16(x[::-1])], axis=-1)                     # interleaved stereo, averaged
            return rs, {"x": st}, lambda rs, dev: {"out": rs.clips(dev["x"], stereo_mode=1)}
        off = offsets_of((3000, 4411, 0, 1, 1589))
        x = noise(off[-1], 52)
        if form == "ragged_pcm16":
            x = pcm16(x)
        return rs, {"x": x}, lambda rs, dev: {"out": rs.ragged(dev["x"], off)[0]}


for _form in ("clips", "clips_pcm16", "ragged", "ragged_pcm16"):
    _resample_case(_form)


# ---- carried state: chains enqueued once behind one delay -------------------------------------------------------------------------------

STREAM_CHUNKS = ((9000, 7000), (8000, 12001), (5000, 0))        # per push, per stream: stream 0 passes 98 rows in the second push


@case("chain_stream_push_x3", "dsp_stream_push_device", reset=lambda sess: sess.reset())
def _(golden):
    import dsp_amd
    plan, stop, spk = _models(golden)
    sess = dsp_amd.StreamSession(plan, 2, stop=stop, speaker=spk, window_frames=98, hop_frames=10)
    inputs = {f"push{p}": noise(sum(lens), 60 + p) for p, lens in enumerate(STREAM_CHUNKS)}

    def run(sess, dev):
        out = {}
        for p, lens in enumerate(STREAM_CHUNKS):
            ro, rows, wo, prob, mean, label = sess.push(dev[f"push{p}"], offsets_of(lens))
            out[f"push{p}"] = [ro, rows, wo, prob, mean, label]
        return out
    return sess, inputs, run


RESAMPLE_CHUNKS = ((4411, 3000), (2999, 5001))


@case("chain_stream_resample_push_x2_finish", ("dsp_stream_resample_push_device", "dsp_stream_resample_finish_device"), reset=lambda rs: rs.reset())
def _(golden):
    from dsp_amd import resample
    rs = resample.StreamResampler(44100, 16000, 2)
    inputs = {f"push{p}": noise(sum(lens), 63 + p) for p, lens in enumerate(RESAMPLE_CHUNKS)}

    def run(rs, dev):
        out = {}
        for p, lens in enumerate(RESAMPLE_CHUNKS):
            out[f"push{p}"] = list(rs.push(dev[f"push{p}"], offsets_of(lens)))
        out["finish"] = list(rs.finish())
        return out
    return rs, inputs, run


def _vad_inputs():
    import dsp_amd
    from tests import vad_util
    cfg = dsp_amd.speaker_config()
    lens = (16000, 0, 4000, 24001)
    off = offsets_of(lens)
    fo = dsp_amd.mfcc.ragged_frame_offsets(cfg, off, 1 << 30)
    return cfg, off, fo, vad_util.signal(71, int(off[-1]))


@case("chain_vad_power_decide_kept_select",
      ("dsp_vad_frame_power_ragged_device", "dsp_vad_decide_ragged_device", "dsp_rows_kept_offsets_device", "dsp_rows_select_ragged_device"),
      waits=("dsp_vad_decide_ragged_device", "dsp_rows_kept_offsets_device"),
      note="decide and kept_offsets fill a HOST array of offsets and wait; select, behind them, has a case of its own for the event")
def _(golden):
    import dsp_amd
    cfg, off, fo, x = _vad_inputs()
    vad = dsp_amd.Vad(cfg, reference="max", threshold_db=-30.0, context_frames=2, pad_frames=1)
    feats = _rows(fo[-1], 13, 72)

    def run(vad, dev):
        power = vad.power(dev["x"], off, fo)
        flags, kept, records, level = vad.decide(power, fo, levels=True)
        kept2 = vad.kept_offsets(flags, fo)
        rows, index = vad.select(dev["feats"], flags, fo, kept2, index=True)
        return {"power": power, "flags": flags, "kept": kept, "records": records, "level": level, "kept2": kept2, "rows": rows, "index": index}
    return vad, {"x": x, "feats": feats}, run


@case("vad_run", "dsp_vad_run_ragged_device", waits="dsp_vad_run_ragged_device")
def _(golden):
    import dsp_amd
    cfg, off, fo, x = _vad_inputs()
    vad = dsp_amd.Vad(cfg, reference="mean", threshold_db=-10.0)
    return vad, {"x": x}, lambda vad, dev: dict(zip(("flags", "kept", "records", "level"), vad.run(dev["x"], off, fo, levels=True)))


@case("rows_select", "dsp_rows_select_ragged_device")
def _(golden):
    import dsp_amd
    cfg = dsp_amd.speaker_config()
    fo = offsets_of((100, 0, 26, 151))
    flags = (np.random.default_rng(73).random(int(fo[-1])) < 0.6).astype(np.uint8)
    kept = np.concatenate([[0], np.cumsum([flags[a:b].sum() for a, b in zip(fo[:-1], fo[1:])])]).astype(np.int64)
    vad = dsp_amd.Vad(cfg)
    feats = _rows(fo[-1], 13, 74)
    return vad, {"feats": feats, "flags": flags}, lambda vad, dev: dict(zip(("rows", "index"), vad.select(dev["feats"], dev["flags"], fo, kept, index=True)))


def _trials_evaluate(ev, scores, truth, n_thresholds):
    """dsp_trials_evaluate_device through ctypes with every output on the device (TrialEvaluator.evaluate copies them to the host)"""
    import torch
    import dsp_amd.lib as dl
    n_rows, n_col = scores.shape
    tr = np.ascontiguousarray(truth, np.intc)
    n_tgt = int((tr >= 0).sum())
    dev = scores.device
    out = {"columns": torch.empty((n_col + 1, 10), dtype=torch.int64, device=dev),
           "tp": torch.empty((n_col + 1, n_thresholds), dtype=torch.int64, device=dev),
           "fp": torch.empty((n_col + 1, n_thresholds), dtype=torch.int64, device=dev),
           "above": torch.empty(max(n_tgt, 1), dtype=torch.int32, device=dev), "equal": torch.empty(max(n_tgt, 1), dtype=torch.int32, device=dev)}
    cfg = dl.TrialsConfig(int(n_thresholds))
    dl.check(ev._L.dsp_trials_evaluate_device(ev._h, scores.data_ptr(), n_rows, n_col, tr.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cfg),
                                              *[out[k].data_ptr() for k in ("columns", "tp", "fp", "above", "equal")], dl.current_stream(scores)),
             "dsp_trials_evaluate_device")
    return out


@case("chain_cmvn_enroll_verify_snorm_calibrate_trials",
      ("dsp_cmvn_ragged_device", "dsp_speaker_enroll_ragged_device", "dsp_speaker_verify_ragged_device", "dsp_cohort_stats_device",
       "dsp_score_normalize_device", "dsp_calibration_apply_device", "dsp_trials_evaluate_device"))
def _(golden):
    import dsp_amd
    from tests import verify_util
    sw = verify_util.sweep_case(5, 13)
    ubm, fo = sw["ubm"], sw["fo"]
    st = {"cmvn": dsp_amd.Cmvn(13, 300), "enroller": dsp_amd.SpeakerEnroller(ubm), "verifier": dsp_amd.SpeakerVerifier(ubm),
          "norm": dsp_amd.ScoreNormalizer(), "cal": dsp_amd.ScoreCalibrator(), "ev": dsp_amd.TrialEvaluator()}
    n = fo.size - 1
    truth = (np.arange(n) % (n + 1) - (np.arange(n) % 4 == 3) * (np.arange(n) + 1)).astype(np.int32)      # own speaker, every fourth clip -1

    def run(st, dev):
        z = st["cmvn"].apply(dev["feats"], fo)
        enrolled = st["enroller"].enroll(z, fo)
        scores = st["verifier"].verify(z, fo, enrolled["means"], want=("llr", "ll_ubm", "ll_target", "best", "best_llr"))
        row, col = st["norm"].stats(scores["llr"], "row"), st["norm"].stats(scores["llr"], "column", top_k=3)
        normed = st["norm"].apply(scores["llr"], "s", row, col)
        cal = st["cal"].apply(normed, (1.25, -0.5, 0.125), n_frames=np.diff(fo))
        trials = _trials_evaluate(st["ev"], cal, truth, 200)
        return {"z": z, "enrolled": enrolled, "scores": scores, "row": row, "col": col, "normed": normed, "cal": cal, "trials": trials}
    return st, {"feats": np.array(sw["feats"])}, run


@case("trials_evaluate", "dsp_trials_evaluate_device")
def _(golden):
    import dsp_amd
    from tests import trials_util
    x, truth = trials_util.case_inputs(65, 5, 1024, "grid", "mixed")
    return dsp_amd.TrialEvaluator(), {"x": np.array(x)}, lambda ev, dev: _trials_evaluate(ev, dev["x"], truth, 1024)


@case("cohort_stats_score_normalize", ("dsp_cohort_stats_device", "dsp_score_normalize_device"))
def _(golden):
    import dsp_amd
    from tests import snorm_util
    cohort = np.array(snorm_util.cohort(65, 64))                    # [64][65]: 64 trial clips against 65 cohort speakers
    scores = np.array(snorm_util.scores(64, 5))

    def run(norm, dev):
        row = norm.stats(dev["cohort"], "row", top_k=30)
        col = norm.stats(dev["cohort"][:, :5].contiguous(), "column")
        return {"row": row, "col": col, "out": norm.apply(dev["scores"], "s", row, col)}
    return dsp_amd.ScoreNormalizer(), {"cohort": cohort, "scores": scores}, run


@case("calibration_fit", "dsp_calibration_fit_device", waits="dsp_calibration_fit_device")
def _(golden):
    import dsp_amd
    from tests import calibration_util
    x, truth, n_frames = calibration_util.case_inputs(257, 3)

    def run(cal, dev):
        rep = cal.fit(dev["x"], truth, n_frames, tol=calibration_util.TOL)
        return {"report": np.array([rep[k] for k in ("a", "b", "c", "objective", "objective_start", "last_step")]),
                "counts": np.array([rep[k] for k in ("n_target", "n_nontarget", "n_excluded", "n_iter", "n_rejected", "status")])}
    return dsp_amd.ScoreCalibrator(), {"x": np.array(x)}, run


def _segments(seg, scores, wo, n_col, cfg):
    """dsp_segments_device through ctypes with the count left on the device (Segmenter.segments reads it on the host)"""
    import torch
    import dsp_amd.lib as dl
    room = dl.check(seg._L.dsp_segments_capacity(C.byref(cfg), wo.ctypes.data_as(dl.LP), wo.size - 1, n_col), "dsp_segments_capacity")
    out = torch.empty((room, 8), dtype=torch.int32, device=scores.device)
    counts = torch.empty((wo.size - 1, n_col), dtype=torch.int32, device=scores.device)
    total = torch.empty(2, dtype=torch.int64, device=scores.device)
    dl.check(seg._L.dsp_segments_device(seg._h, scores.data_ptr(), wo.size - 1, wo.ctypes.data_as(dl.LP), n_col, C.byref(cfg), out.data_ptr(), room,
                                        counts.data_ptr(), total.data_ptr(), dl.current_stream(scores)), "dsp_segments_device")
    return {"segments": out, "counts": counts, "total": total}


@case("chain_speaker_float_scan_segments", ("dsp_speaker_float_scan_device", "dsp_segments_device"))
def _(golden):
    import dsp_amd
    import dsp_amd.lib as dl
    from dsp_amd import consumers
    from tests import verify_util
    sw = verify_util.sweep_case(5, 13)
    fo = sw["fo"]
    wo = consumers.scan_window_offsets(fo, 30, 7)
    cfg = dl.SegmentConfig(0.0, -0.5, 2, 1, dl.SEG_INDEPENDENT)
    st = {"verifier": dsp_amd.SpeakerVerifier(sw["ubm"]), "seg": dsp_amd.Segmenter()}

    def run(st, dev):
        scan = st["verifier"].scan(dev["feats"], fo, dev["means"], 30, 7, want=("llr", "ll_ubm", "ll_target", "best", "best_llr"))
        return {"scan": scan, "segments": _segments(st["seg"], scan["llr"], wo, 5, cfg)}
    return st, {"feats": np.array(sw["feats"]), "means": np.array(sw["means"][:5])}, run


AUGMENT_CLIPS = (1025, 2049)


@case("chain_stft_istft_stretch_augment",
      ("dsp_stft_ragged_device", "dsp_istft_ragged_device", "dsp_time_stretch_ragged_device", "dsp_augment_ragged_device"))
def _(golden):
    from dsp_amd import augment
    aug = augment.Augmenter()
    off = offsets_of(AUGMENT_CLIPS)
    ops = augment.make_ops([dict(clip=0, kind="stretch", rate=1.1), dict(clip=1, kind="pitch", n_steps=2), dict(clip=0, kind="noise", sigma=0.005, key=3)])

    def run(aug, dev):
        spec, fo = aug.stft(dev["x"], off)
        back, _ = aug.istft(spec, fo, np.diff(off))
        stretched, so = aug.time_stretch(dev["x"], off, [1.25, 0.8])
        augmented, ao = aug.apply(dev["x"], off, ops, seed=5)
        return {"spec": spec, "fo": fo, "back": back, "stretched": stretched, "so": so, "augmented": augmented, "ao": ao}
    return aug, {"x": noise(off[-1], 81)}, run


# ---- training entries: documented to wait; each case's first kernels sit behind the delay -------------------------------------------------

UBM_K, UBM_D, UBM_N = 4, 13, 700


def _ubm_rows():
    rng = np.random.default_rng(91)
    centres = rng.normal(0.0, 2.0, (UBM_K, UBM_D))
    return (centres[rng.integers(UBM_K, size=UBM_N)] + rng.normal(0.0, 0.7, (UBM_N, UBM_D))).astype(np.float32)


def _ubm_case(id, name, call):
    @case(id, name, waits=name)
    def build(golden):
        import dsp_amd
        return dsp_amd.UbmTrainer(UBM_K, UBM_D), {"x": _ubm_rows()}, lambda t, dev: call(t, dev["x"])


def _fit_outputs(r):
    return {k: v for k, v in r.items() if k != "report"} | ({"winner": r["report"]["winner"], "restarts": [sorted(x.items()) for x in r["report"]["restarts"]]}
                                                           if "report" in r else {})


_ubm_case("ubm_init_rows", "dsp_ubm_init_rows_device", lambda t, x: t.init_rows(x))
_ubm_case("ubm_train", "dsp_ubm_train_device", lambda t, x: _fit_outputs(t.fit(x, max_iter=5, tol=0.0)))
_ubm_case("kmeans_seed", "dsp_kmeans_seed_device", lambda t, x: {"rows": t.kmeans_seed(x, seed=7)})
_ubm_case("kmeans_fit", "dsp_kmeans_fit_device",
          lambda t, x: {k: v for k, v in t.kmeans(x, _ubm_rows().astype(np.float64)[[10, 200, 400, 650]], max_iter=8, want_labels=True).items() if k != "stop"})
_ubm_case("kmeans_train_ubm", "dsp_kmeans_train_ubm_device",
          lambda t, x: _fit_outputs(t.fit(x, init="kmeans", n_init=2, seed=3, max_iter=3, tol=0.0, kmeans_max_iter=5)))


def _svm_data():
    rng = np.random.default_rng(92)
    labels = (np.arange(60) % 2).astype(np.int32)
    x = (rng.standard_normal((60, 40)) + 0.8 * (2 * labels[:, None] - 1) * (np.arange(40) < 6)).astype(np.float32)
    return x, labels


@case("svm_train_set", "dsp_svm_train_set_device", waits="dsp_svm_train_set_device")
def _(golden):
    from dsp_amd import scrubjay
    x, _labels = _svm_data()
    t = scrubjay.SvmTrainer(40)

    def run(t, dev):
        off, scl = t.set(dev["x"])
        return {"offset": off, "scale": scl, "z": t.rows()}
    return t, {"x": x}, run


@case("svm_train_problems", "dsp_svm_train_problems_device", waits="dsp_svm_train_problems_device",
      note="the dataset is set before the case runs: the entry's device inputs are the trainer's own")
def _(golden):
    import torch
    from dsp_amd import scrubjay
    x, labels = _svm_data()
    t = scrubjay.SvmTrainer(40)
    t.set(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    problems = [(np.arange(60), 10.0, 10.0, 0.02), (np.arange(0, 60, 2), 1.0, 1.0, 0.02), (np.arange(1, 50), 3.0, 5.0, 0.1)]

    def run(t, dev):
        res, coef, dec = t.problems(problems, labels)
        return {"results": res, "coef": coef, "dec": dec}
    return t, {}, run


@case("svm_platt_fit", "dsp_svm_platt_fit_device", waits="dsp_svm_platt_fit_device")
def _(golden):
    import torch
    from dsp_amd import scrubjay
    x, labels = _svm_data()
    t = scrubjay.SvmTrainer(40)
    t.set(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    dec = (np.random.default_rng(93).standard_normal(60) + 1.5 * (1 - 2 * labels)).astype(np.float64)
    return t, {"dec": dec}, lambda t, dev: {"platt": np.array(t.platt(dev["dec"], labels), np.float64)}


@case("svm_fit", "dsp_svm_fit_device", waits="dsp_svm_fit_device")
def _(golden):
    from dsp_amd import scrubjay
    x, labels = _svm_data()
    t = scrubjay.SvmTrainer(40)

    def run(t, dev):
        attrs, report = t.fit(dev["x"], labels, C=10.0, gamma=0.02, probability_folds=3, seed=1)
        return {"attrs": attrs, "report": [report[k] for k in ("n_sv", "n_iter", "n_bounded", "objective", "gap", "rho", "platt_iter")]}
    return t, {"x": x}, run


def _stop_train_case():
    from tests import stoptrain_ref
    return stoptrain_ref.case("A")


@case("stop_train_set", "dsp_stop_train_set_device", waits="dsp_stop_train_set_device")
def _(golden):
    import dsp_amd
    c = _stop_train_case()
    t = dsp_amd.StopTrainer(c["n_coef"], c["max_frames"], c["units"])

    def run(t, dev):
        mean, scale = t.set(dev["mfcc"], c["frame_offsets"], scaler_rows=c["train_rows"])
        return {"mean": mean, "scale": scale, "z": t.rows()}
    return t, {"mfcc": np.array(c["mfcc"])}, run


@case("stop_train_runs", "dsp_stop_train_runs_device", waits="dsp_stop_train_runs_device",
      note="the dataset is set before the case runs: the entry's device inputs are the trainer's own")
def _(golden):
    import torch
    import dsp_amd
    c = _stop_train_case()
    t = dsp_amd.StopTrainer(c["n_coef"], c["max_frames"], c["units"])
    t.set(torch.from_numpy(np.ascontiguousarray(c["mfcc"])).cuda(), c["frame_offsets"], scaler_rows=c["train_rows"])
    torch.cuda.synchronize()

    def run(t, dev):
        res, hist, prob, params = t.train(c["runs"], c["labels"])
        return {"results": res, "history": hist, "prob": prob, "params": params}
    return t, {}, run
