"""GPU: voice activity detection (dsp_vad_*, dsp_rows_*; dsp_amd.Vad) against the float64 restatement of
tests/vad_ref.py, bit for bit, through the raw C entries and through the Python class.  Every output buffer is filled with a sentinel
beforehand and followed by spare entries that must keep it."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import vad_ref as V
from tests import vad_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dsp_amd")
LP = dl.LP
SPARE = 8
TILE = V.TILE
# beside the issue's four: a sub-block no multiple of 4 samples (dword loads only), frames that do not touch (hop > frame_length), and
# one whose rows of a tile do not fit the LDS image at once (chunks of 227 rows)
MORE_FRAMINGS = {"30/10 complete": (30, 10, V.COMPLETE), "64/160 complete": (64, 160, V.COMPLETE), "160/144 complete": (160, 144, V.COMPLETE)}
ALL_FRAMINGS = {**U.FRAMINGS, **MORE_FRAMINGS}


def _torch():
    import torch
    return torch


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _workspace(n, rows, fill=0xA5):
    torch = _torch()
    need = dl.load().dsp_vad_workspace_bytes(n, rows)
    assert need > 0
    return torch.full((need,), fill, dtype=torch.uint8, device="cuda"), need


def _lp(a):
    return a.ctypes.data_as(LP)


class Batch:
    """clips of the wanted row counts, back to back: signal, offsets, frame_offsets"""

    def __init__(self, framing, rows, extras, seed=11):
        fl, hop, kind = framing
        lengths = [U.samples_for(r, fl, hop, kind, e % hop) for r, e in zip(rows, extras)]
        assert [V.frames_for(n, fl, hop, kind) for n in lengths] == list(rows)
        self.framing = framing
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self.frame_offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        self.signal = U.signal(seed, int(self.offsets[-1]))
        self.n, self.R = len(rows), int(self.frame_offsets[-1])
        self.rows = self.R

    def device(self):
        return _torch().from_numpy(self.signal).cuda()


def _power_batch(name):
    fl, hop, kind = framing = ALL_FRAMINGS[name]
    geo = U.geometry(U.config(fl, hop, kind, context=64, pad=64))
    assert geo.rows_per_tile == TILE and geo.halo_rows == 128
    rows = [2 * TILE + geo.halo_rows + 1, 0, 1, 2, TILE - 1, TILE, TILE + 1, 0, 3]
    extras = [0, 0, 7, 4, 1, 0, 3, 0, 0]              # lengths that are no multiple of g; clip starts at multiples of 4 and at odd samples
    b = Batch(framing, rows, extras)
    g = geo.g
    assert any(n % g for n in np.diff(b.offsets)) and {int(o) % 4 == 0 for o in b.offsets[:-1]} == {True, False} and any(int(o) % 2 for o in b.offsets)
    return b


_reference = {}


def _ref_power(name):
    if name not in _reference:
        b = _power_batch(name)
        fl, hop, kind = b.framing
        P = np.zeros(b.R, np.float64)
        for c in range(b.n):
            a, e = b.frame_offsets[c], b.frame_offsets[c + 1]
            P[a:e] = V.frame_power(b.signal[b.offsets[c]:b.offsets[c + 1]], fl, hop, kind, e - a)
        _reference[name] = (b, P)
    return _reference[name]


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- 1. frame power ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(ALL_FRAMINGS))
def test_frame_power_bit_for_bit(name):
    torch = _torch()
    L = dsp_amd.load()
    b, want = _ref_power(name)
    cfg = U.config(*b.framing)
    sig = b.device()
    out = torch.full((b.R + SPARE,), -7.0, dtype=torch.float64, device="cuda")
    ws, ws_bytes = _workspace(b.n, b.rows)
    rc = L.dsp_vad_frame_power_ragged_device(0, C.byref(cfg), sig.data_ptr(), b.n, _lp(b.offsets), _lp(b.frame_offsets), out.data_ptr(), ws.data_ptr(), ws_bytes,
                                             _stream())
    assert rc == 0, dl.last_error()
    got = out.cpu().numpy()
    assert (got[b.R:] == -7.0).all()
    assert _same_bits(got[:b.R], want), f"{name}: {np.flatnonzero(got[:b.R] != want)[:8]}"
    assert (want > 0).all()
    with dsp_amd.Vad(dsp_amd.default_config(frame_length=b.framing[0], hop_length=b.framing[1], framing=b.framing[2])) as v:     # and through the class
        assert _same_bits(v.power(sig, b.offsets, b.frame_offsets).cpu().numpy(), want)


def test_frame_power_of_fewer_rows_than_the_clip_gives():
    """a max_frames cap: the first rows of the same clip"""
    b, want = _ref_power("400/160 centre")
    with dsp_amd.Vad(dsp_amd.speaker_config()) as v:
        fo = np.array([0, 100], np.int64)
        got = v.power(b.device(), b.offsets[:2], fo).cpu().numpy()
    assert _same_bits(got, want[:100])


# ---- 2. the decision --------------------------------------------------------------------------------------------------------------

RATIOS = {"absolute": 1e-3, "max": 1e-2, "mean": 0.5}


def _decision_signal(hop, rows):
    """a clip of `rows` rows under 400/160 centre: noise, with loud runs that touch both ends and straddle the tiles' edges"""
    rng = np.random.default_rng(rows)
    x = rng.normal(0.0, 1e-3, (rows - 1) * hop)
    for a, e in ((0, 4), (250, 259), (300, 301), (508, 516), (rows - 5, rows)):
        if a < rows:
            x[a * hop:min(e, rows - 1) * hop] += rng.normal(0.0, 0.3, min(e, rows - 1) * hop - a * hop)
    return x.astype(np.float32)


def _decision_batch():
    """400/160 centre: the constructed clip over three tiles and a halo, an all-zero clip, an all-speech clip, a clip holding NaN and inf
    samples, a loud clip beside a silent one, a clip without rows and short clips, from row 5 and sample 3 on"""
    hop = 160
    rng = np.random.default_rng(3)
    big = 2 * TILE + 128 + 1
    nan_clip = _decision_signal(hop, 300)
    nan_clip[1000], nan_clip[30000], nan_clip[30001] = np.nan, np.inf, -np.inf
    clips = [_decision_signal(hop, big), np.zeros(299 * hop, np.float32), rng.normal(0.0, 0.2, 256 * hop).astype(np.float32), nan_clip,
             rng.normal(0.0, 0.4, 40 * hop).astype(np.float32), rng.normal(0.0, 1e-3, 40 * hop + 7).astype(np.float32), np.zeros(0, np.float32),
             _decision_signal(hop, TILE), _decision_signal(hop, TILE + 1), rng.normal(0.0, 0.1, 5).astype(np.float32)]
    lengths = [c.size for c in clips]
    offsets = 3 + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    signal = np.concatenate([np.full(3, 9.0, np.float32)] + clips)
    fo = 5 + np.concatenate([[0], np.cumsum([V.frames_for(n, 400, hop, V.CENTER) for n in lengths])]).astype(np.int64)
    return signal, offsets, fo


_decisions = {}


def _ref_decision(reference, context, pad):
    key = (reference, context, pad)
    if "batch" not in _decisions:
        signal, offsets, fo = _decision_batch()
        P = np.zeros(int(fo[-1]), np.float64)
        for c in range(offsets.size - 1):
            P[fo[c]:fo[c + 1]] = V.frame_power(signal[offsets[c]:offsets[c + 1]], 400, 160, V.CENTER)
        _decisions["batch"] = (signal, offsets, fo, P)
    signal, offsets, fo, P = _decisions["batch"]
    if key not in _decisions:
        cfg = U.config(400, 160, V.CENTER, U.REFERENCES[reference], RATIOS[reference], 1e-7, context, 0.6, pad)
        n = offsets.size - 1
        flags, level = np.zeros(int(fo[-1]), np.uint8), np.zeros(int(fo[-1]), np.float32)
        records, kept = np.zeros(n, V.CLIP_DTYPE), np.zeros(n + 1, np.int64)
        for c in range(n):
            flags[fo[c]:fo[c + 1]], records[c], _, level[fo[c]:fo[c + 1]] = V.decide(P[fo[c]:fo[c + 1]], **U.how(cfg))
            kept[c + 1] = kept[c] + records[c]["n_kept"]
        _decisions[key] = (cfg, flags, records, kept, level)
    return (signal, offsets, fo, P) + _decisions[key]


def _ordered(x):
    """float32 -> integers that grow with the float, one step per representable value"""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _levels_agree(got, want):
    """within one float32 step of the float64 value rounded to float32 (the device's float64 log10 is a few float64 ulp off, which can
    move the float32 rounding by one step at most); non-finite values of the same kind"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    assert (np.abs(_ordered(got[fin]) - _ordered(want[fin])) <= 1).all()


@pytest.mark.parametrize("context,pad", [(0, 0), (5, 0), (0, 3), (64, 64)])
@pytest.mark.parametrize("reference", list(U.REFERENCES))
def test_flags_records_and_kept_offsets_bit_for_bit(reference, context, pad):
    torch = _torch()
    L = dsp_amd.load()
    signal, offsets, fo, P, cfg, flags, records, kept, level = _ref_decision(reference, context, pad)
    n, R, rows = offsets.size - 1, int(fo[-1]), int(fo[-1] - fo[0])
    assert records["n_kept"][1] == 0 and records["n_kept"][2] >= 250 and records["n_raw"][3] > 0 and not np.isfinite(P[fo[3]:fo[4]]).all()
    if (context, pad) == (0, 0):
        assert np.array_equal(records["n_raw"], records["n_kept"])
        assert flags[fo[0]] and flags[fo[1] - 1] and flags[fo[0] + 255] and flags[fo[0] + 256] and not flags[fo[0] + 262]      # runs at the ends and over a tile's edge
    sig = torch.from_numpy(signal).cuda()
    power = torch.from_numpy(P).cuda()
    for entry in ("decide", "run"):
        d_flags = torch.full((R + SPARE,), 0xCC, dtype=torch.uint8, device="cuda")
        d_level = torch.full((R + SPARE,), -7.0, dtype=torch.float32, device="cuda")
        d_clips = torch.full((n + 2, 4), -1, dtype=torch.int64, device="cuda")
        ko = np.full(n + 1 + 2, -5, np.int64)
        ws, ws_bytes = _workspace(n, rows, 0x5A if entry == "run" else 0xFF)
        if entry == "decide":
            rc = L.dsp_vad_decide_ragged_device(0, C.byref(cfg), power.data_ptr(), n, _lp(fo), d_flags.data_ptr(), d_level.data_ptr(), d_clips.data_ptr(), _lp(ko),
                                                ws.data_ptr(), ws_bytes, _stream())
        else:
            rc = L.dsp_vad_run_ragged_device(0, C.byref(cfg), sig.data_ptr(), n, _lp(offsets), _lp(fo), d_flags.data_ptr(), d_level.data_ptr(), d_clips.data_ptr(),
                                             _lp(ko), ws.data_ptr(), ws_bytes, _stream())
        assert rc == 0, dl.last_error()
        got_flags, got_level, got_clips = d_flags.cpu().numpy(), d_level.cpu().numpy(), d_clips.cpu().numpy()
        assert (got_flags[:5] == 0xCC).all() and (got_flags[R:] == 0xCC).all() and (got_level[:5] == -7.0).all() and (got_level[R:] == -7.0).all()
        assert (got_clips[n:] == -1).all() and (ko[n + 1:] == -5).all()
        assert np.array_equal(got_flags[5:R], flags[5:]), entry
        got_records = got_clips[:n].view(V.CLIP_DTYPE).reshape(-1)
        assert _same_bits(got_records, records), (entry, got_records, records)
        assert np.array_equal(ko[:n + 1], kept)
        _levels_agree(got_level[5:R], level[5:])
    with dsp_amd.Vad(dsp_amd.speaker_config(), reference, 10.0 * np.log10(RATIOS[reference]), -70.0, context, 0.6, pad) as v:      # and through the class
        assert abs(v.cfg.threshold_ratio / cfg.threshold_ratio - 1.0) < 1e-12
        v.cfg.threshold_ratio, v.cfg.floor_power = cfg.threshold_ratio, cfg.floor_power          # (pow's last bit is not what is tested here)
        f, k, r, lv = v.run(sig, offsets, fo, levels=True)
        assert np.array_equal(f.cpu().numpy()[5:], flags[5:]) and np.array_equal(k, kept) and _same_bits(r, records)
        _levels_agree(lv.cpu().numpy()[5:], level[5:])
        f2, k2, r2 = v.decide(power, fo)
        assert torch.equal(f, f2) and np.array_equal(k2, kept) and _same_bits(r2, records)
        starts, lengths, with_speech = v.trim_spans(records, offsets)
        want = V.trim_spans(records, offsets, 160)
        assert np.array_equal(starts, want[0]) and np.array_equal(lengths, want[1]) and with_speech == want[2] == int((records["n_kept"] > 0).sum())


# ---- 3. the selection -------------------------------------------------------------------------------------------------------------


def _select_raw(x, d, flags, fo, ko):
    """dsp_rows_select_ragged_device on numpy inputs -> (rows, row_index), with the sentinels checked"""
    torch = _torch()
    L = dsp_amd.load()
    n, kept = fo.size - 1, int(ko[-1])
    d_in, d_flags = torch.from_numpy(x).cuda(), torch.from_numpy(flags).cuda()
    out = torch.full(((kept + SPARE) * d,), -7.0, dtype=torch.float32, device="cuda")
    index = torch.full((kept + SPARE,), -9, dtype=torch.int64, device="cuda")
    ws, ws_bytes = _workspace(n, int(fo[-1] - fo[0]))
    rc = L.dsp_rows_select_ragged_device(0, d_in.data_ptr(), d, d_flags.data_ptr(), n, _lp(fo), _lp(ko), out.data_ptr(), index.data_ptr(), ws.data_ptr(), ws_bytes,
                                         _stream())
    assert rc == 0, dl.last_error()
    out, index = out.cpu().numpy(), index.cpu().numpy()
    assert (out[kept * d:] == -7.0).all() and (index[kept:] == -9).all()
    return out[:kept * d].reshape(kept, d), index[:kept]


def _kept_offsets_raw(flags, fo):
    torch = _torch()
    L = dsp_amd.load()
    n = fo.size - 1
    ko = np.full(n + 1 + 2, -5, np.int64)
    ws, ws_bytes = _workspace(n, int(fo[-1] - fo[0]))
    d_flags = torch.from_numpy(flags).cuda()
    rc = L.dsp_rows_kept_offsets_device(0, d_flags.data_ptr(), n, _lp(fo), _lp(ko), ws.data_ptr(), ws_bytes, _stream())
    assert rc == 0, dl.last_error()
    assert (ko[n + 1:] == -5).all()
    return ko[:n + 1].copy()


@pytest.mark.parametrize("d", [1, 13, 16, 64])
def test_selection_equals_numpy(d):
    _, _, fo, _, _, vad_flags, _, vad_kept, _ = _ref_decision("max", 5, 0)
    R = int(fo[-1])
    rng = np.random.default_rng(d)
    x = rng.normal(0.0, 1.0, (R, d)).astype(np.float32)
    inside = np.zeros(R, bool)
    inside[5:] = True
    user = {"zeros": np.zeros(R, np.uint8), "ones": np.ones(R, np.uint8), "alternating": (np.arange(R) % 2).astype(np.uint8),
            "bytes": np.where(rng.random(R) < 0.3, rng.integers(1, 256, R), 0).astype(np.uint8)}
    for name, flags in [("vad", vad_flags)] + list(user.items()):
        want_ko = np.concatenate([[0], np.cumsum([np.count_nonzero(flags[fo[c]:fo[c + 1]]) for c in range(fo.size - 1)])]).astype(np.int64)
        ko = _kept_offsets_raw(flags, fo)
        assert np.array_equal(ko, want_ko), name
        if name == "vad":
            assert np.array_equal(ko, vad_kept)
        rows, index = _select_raw(x, d, flags, fo, ko)
        keep = (flags != 0) & inside
        assert _same_bits(rows, x[keep]) and np.array_equal(index, np.flatnonzero(keep)), name
    with dsp_amd.Vad(dsp_amd.speaker_config()) as v:
        torch = _torch()
        flags = torch.from_numpy(user["alternating"]).cuda()
        ko = v.kept_offsets(flags, fo)
        got, index = v.select(torch.from_numpy(x).cuda() if d > 1 else torch.from_numpy(x[:, 0].copy()).cuda(), flags, fo, ko, index=True)
        keep = (user["alternating"] != 0) & inside
        assert _same_bits(got.cpu().numpy().reshape(-1, d), x[keep]) and np.array_equal(index.cpu().numpy(), np.flatnonzero(keep))


# ---- 4. independence --------------------------------------------------------------------------------------------------------------


def _run_all(v, signal, offsets, fo):
    """every output of the chain for one batch, per clip: (power, flags, level, record)"""
    torch = _torch()
    sig = torch.from_numpy(signal).cuda()
    P = v.power(sig, offsets, fo)
    flags, kept, records, level = v.run(sig, offsets, fo, levels=True)
    P, flags, level = P.cpu().numpy(), flags.cpu().numpy(), level.cpu().numpy()
    return [(P[fo[c]:fo[c + 1]].tobytes(), flags[fo[c]:fo[c + 1]].tobytes(), level[fo[c]:fo[c + 1]].tobytes(), records[c].tobytes(), int(kept[c + 1] - kept[c]))
            for c in range(offsets.size - 1)]


def test_a_clip_is_the_same_bits_alone_in_a_batch_reversed_and_on_a_side_stream():
    torch = _torch()
    rng = np.random.default_rng(40)
    lengths = rng.integers(1, 9000, 40)
    lengths[7], lengths[20] = 2 * TILE * 160 + 77, 0
    clips = [U.signal(100 + i, int(n)) for i, n in enumerate(lengths)]

    def batch(order, lead):
        """the clips in `order` behind `lead` samples that belong to no clip: a clip's start changes its alignment and so its load form"""
        signal = np.concatenate([np.full(lead, 5.0, np.float32)] + [clips[i] for i in order])
        offsets = lead + np.concatenate([[0], np.cumsum([clips[i].size for i in order])]).astype(np.int64)
        fo = np.concatenate([[0], np.cumsum([V.frames_for(clips[i].size, 400, 160, V.CENTER) for i in order])]).astype(np.int64)
        return signal, offsets, fo

    order = list(range(40))
    for reference in ("max", "mean"):
        with dsp_amd.Vad(dsp_amd.speaker_config(), reference, -20.0 if reference == "max" else -3.0, context_frames=5, pad_frames=3) as v:
            whole = _run_all(v, *batch(order, 0))
            back = _run_all(v, *batch(order[::-1], 3))
            assert back[::-1] == whole
            for i in (0, 7, 20, 39):
                for lead in (0, 1, 4):
                    assert _run_all(v, *batch([i], lead)) == [whole[i]], (reference, i, lead)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                v._workspace(40, 100000)
                v._ws.fill_(0xEE)                                     # what the workspace held must not matter
                again = _run_all(v, *batch(order, 0))
            side.synchronize()
            assert again == whole


# ---- 5. the chain -----------------------------------------------------------------------------------------------------------------


def _speech_like(seed, seconds, bursts):
    """noise at 1e-3 with loud stretches (seconds as (start, stop) pairs)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1e-3, int(seconds * 16000))
    t = np.arange(x.size) / 16000.0
    for a, e in bursts:
        on = (t >= a) & (t < e)
        x[on] += 0.2 * np.sin(2 * np.pi * (200.0 + 40.0 * seed) * t[on]) + rng.normal(0.0, 0.1, int(on.sum()))
    return x.astype(np.float32)


def test_the_front_end_selects_after_cmvn_and_the_models_take_the_rows(golden):
    torch = _torch()
    from tests import enroll_util
    _, ubm, _ = enroll_util.fixture(golden)
    clips = [_speech_like(1, 1.5, [(0.4, 1.0)]), _speech_like(2, 1.0, [(0.0, 0.3), (0.6, 0.9)]), _speech_like(3, 1.2, [(0.5, 1.2)])]
    offsets = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    sig = torch.from_numpy(np.concatenate(clips)).cuda()
    with dsp_amd.SpeakerFrontEnd() as fe, dsp_amd.Vad(fe.plan, threshold_db=-20.0, pad_frames=2) as v:
        feats, fo = fe.features(sig, offsets)
        flags, kept, records = v.run(sig, offsets, fo)
        sel, ko = fe.features(sig, offsets, vad=v)
        assert np.array_equal(ko, kept) and 0 < kept[-1] < fo[-1] and (np.diff(kept) > 0).all()
        assert torch.equal(sel, feats[flags.bool()])
        with dsp_amd.SpeakerEnroller(ubm) as en, dsp_amd.SpeakerVerifier(ubm) as ver:
            llr_all = ver.verify(feats, fo, en.enroll(feats, fo)["means"], want=("llr",))["llr"].cpu().numpy()
            llr_sel = ver.verify(sel, ko, en.enroll(sel, ko)["means"], want=("llr",))["llr"].cpu().numpy()
        assert llr_all.shape == llr_sel.shape == (3, 3) and np.isfinite(llr_sel).all() and not np.array_equal(llr_all, llr_sel)
        silent = np.concatenate([clips[0], np.zeros(8000, np.float32), clips[2]])
        with pytest.raises(ValueError, match="clip 1 keeps no row"):
            fe.features(torch.from_numpy(silent).cuda(), [0, clips[0].size, clips[0].size + 8000, silent.size], vad=v)


def test_the_level_track_through_the_segmenter_yields_the_bursts():
    torch = _torch()
    bursts = [(0.5, 1.0), (1.04, 1.5), (2.5, 2.6), (3.0, 3.8)]           # a 40 ms gap to merge, a 100 ms burst to keep, silence between
    x = _speech_like(4, 4.5, bursts)
    offsets = np.array([0, x.size], np.int64)
    with dsp_amd.Vad(dsp_amd.speaker_config(), threshold_db=-20.0) as v, dsp_amd.Segmenter() as seg:
        fo = dsp_amd.ragged_frame_offsets(dsp_amd.speaker_config(), offsets, 2**31 - 1)
        _, _, _, level = v.run(torch.from_numpy(x).cuda(), offsets, fo, levels=True)
        found = seg.segments(level, fo, on=3.0, off=0.0, min_windows=5, max_gap=8)
    spans = [(int(s["first_window"]) * 0.01, (int(s["first_window"]) + int(s["n_windows"])) * 0.01) for s in found]
    want = [(0.5, 1.5), (2.5, 2.6), (3.0, 3.8)]
    assert len(spans) == len(want), spans
    for (a, e), (wa, we) in zip(spans, want):                             # a row's frame reaches 12.5 ms to either side of its centre
        assert abs(a - wa) <= 0.03 and abs(e - we) <= 0.03, spans


# ---- 6. the C caller --------------------------------------------------------------------------------------------------------------


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_c_caller_keeps_the_rows_the_python_wrapper_keeps(tmp_path, golden):
    torch = _torch()
    from tests import enroll_util
    dsp_amd.load()
    exe = str(tmp_path / "main_vad")
    cmd = ["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
           os.path.join(ROOT, "examples", "main_vad.c"), f"-L{LIBDIR}", "-ldsp_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    clips = [_speech_like(1, 1.5, [(0.4, 1.0)]), _speech_like(2, 1.0, [(0.0, 0.3), (0.6, 0.9)])]
    paths = []
    for i, c in enumerate(clips):
        paths.append(str(tmp_path / f"clip{i}.wav"))
        enroll_util.write_wav(paths[-1], np.round(c * 32767.0).astype(np.int16))
    _, ubm, _ = enroll_util.fixture(golden)
    ubm_path = str(tmp_path / "ubm.txt")
    with open(ubm_path, "w") as f:
        f.write("%d %d\n" % ubm["means"].shape)
        for key in ("log_consts", "means", "inv_covs"):
            f.write(" ".join(repr(float(v)) for v in np.ravel(ubm[key])) + "\n")
    r = subprocess.run([exe, "-t", "-20", "-p", "2", "-u", ubm_path] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pcm = [np.round(c * 32767.0).astype(np.int16).astype(np.float32) / 32768.0 for c in clips]
    offsets = np.concatenate([[0], np.cumsum([c.size for c in pcm])]).astype(np.int64)
    with dsp_amd.SpeakerFrontEnd() as fe, dsp_amd.Vad(fe.plan, threshold_db=-20.0, pad_frames=2) as v:
        sig = torch.from_numpy(np.concatenate(pcm)).cuda()
        _, fo = fe.features(sig, offsets)
        _, kept, records = v.run(sig, offsets, fo)
    lines = [line for line in r.stdout.splitlines() if line.startswith("clip ")]
    assert len(lines) == 2
    for c, line in enumerate(lines):
        assert f"clip {c}: {int(fo[c + 1] - fo[c])} rows, {int(records['n_kept'][c])} kept, rows {int(records['first_kept'][c])} .. {int(records['last_kept'][c])}" in line
    assert f"enrolled on {int(kept[-1])} of {int(fo[-1])} rows" in r.stdout
