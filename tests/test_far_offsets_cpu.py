"""No GPU: the table of tests/far_offsets.py against include/dsp_amd.h.  Every dsp_*_device entry point that takes a stride, a HOST array
of offsets, or a row count named in FAR_BY_COUNT is listed in exactly one of: a case's names, NOT_REACHED (with the measured time and a
reason) or EXEMPT (with a reason); every listed name is declared; and every position a case declares straddles or passes its boundary,
lies inside the arena's payload and keeps the compact call's alignment.  An entry added later with a stride and no case fails here."""
import os
import re

from tests import far_offsets as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = re.compile(r"\b(dsp_\w+_device(?:_f64|_cfg|_ctx)?)\s*\(([^;{}]*?)\)\s*;", re.S)
OFFSETS = ("offsets", "frame_offsets", "window_offsets", "chunk_offsets")

# row- or frame-major inputs whose n x width crosses 2^31 with neither a stride nor (for the first five) an offsets array
FAR_BY_COUNT = ("dsp_mfcc_frames_device", "dsp_stop_predict_device", "dsp_speaker_llr_device", "dsp_speaker_llr_ragged_device", "dsp_mfcc_stats_device",
                "dsp_cmvn_ragged_device", "dsp_speaker_verify_ragged_device", "dsp_speaker_enroll_ragged_device", "dsp_stop_scan_device",
                "dsp_speaker_scan_device", "dsp_svm_scan_device", "dsp_speaker_float_scan_device", "dsp_rows_select_ragged_device")


def _declared():
    """device entry point -> [(type, name)] of its parameters, from the header with its comments blanked"""
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        code = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    out = {}
    for m in DECL.finditer(code):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            name = re.search(r"(\w+)\s*(?:\[\w*\])?$", p).group(1)
            params.append((p[:p.rindex(name)].strip(), name))
        out[m.group(1)] = params
    return out


def _required(declared):
    need = set(FAR_BY_COUNT)
    for entry, params in declared.items():
        for type_, name in params:
            if name.endswith("stride") or (name in OFFSETS and type_.replace(" ", "") == "constlong*"):
                need.add(entry)
    return need


def test_the_parse_finds_the_entries():
    declared = _declared()
    assert len(declared) >= 73                       # the count when the table was written, dsp_classify_batch_device_ctx included
    assert ("long", "clip_stride") in declared["dsp_mfcc_clips_device"]
    assert ("const long *", "offsets") in declared["dsp_mfcc_clips_ragged_device"]
    assert ("const long *", "frame_offsets") in declared["dsp_stop_train_set_device"]           # (a comment inside the parameter list)
    assert ("long", "out_stride") in declared["dsp_resample_clips_device"]
    need = _required(declared)
    assert set(FAR_BY_COUNT) <= set(declared)
    assert "dsp_classify_batch_device_ctx" in need and "dsp_svm_predict_device" not in need and len(need) == 56


def test_every_strided_or_ragged_entry_is_listed_once():
    declared = _declared()
    places = {"a case": set(FO.covered()), "NOT_REACHED": set(FO.NOT_REACHED), "EXEMPT": set(FO.EXEMPT)}
    for a in places:
        for b in places:
            if a < b:
                assert not places[a] & places[b], f"listed in {a} and in {b}: {sorted(places[a] & places[b])}"
    listed = set().union(*places.values())
    missing = sorted(_required(declared) - listed)
    assert not missing, f"device entry points with a stride, offsets or a far row count and no far-offsets case: {missing}"
    unknown = sorted(listed - set(declared))
    assert not unknown, f"listed, but not declared in the header: {unknown}"


def test_every_exemption_carries_its_reason():
    for name, reason in FO.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) > 20, name
    for name, (ms, reason) in FO.NOT_REACHED.items():
        assert isinstance(reason, str) and len(reason.strip()) > 20, name
        assert ms is None or ms > FO.LIMIT_MS, f"{name}: measured at {ms} ms, under the limit: it gets a case"


def test_the_cases_are_well_formed():
    ids = [c.id for c in FO.CASES]
    assert len(ids) == len(set(ids))
    for c in FO.CASES:
        assert c.names and c.group in "ABCD" and c.id.startswith(c.group + "_") and c.elem in FO.ELEM_BYTES and c.layouts, c.id


def test_groups_a_and_b_are_complete():
    """the entries the two mandatory groups name, each in a case of its group"""
    by_group = {g: {n for c in FO.CASES if c.group == g for n in c.names} for g in "AB"}
    assert by_group["A"] >= {
        "dsp_mfcc_clips_device", "dsp_mfcc_clips_pcm16_device", "dsp_classify_batch_device", "dsp_classify_batch_device_cfg", "dsp_classify_batch_device_ctx",
        "dsp_classify_batch_pcm16_device", "dsp_classify_batch_device_f64", "dsp_classify_batch_pcm16_device_f64", "dsp_scrubjay_fused_device",
        "dsp_scrubjay_fused_pcm16_device", "dsp_classify_signal_batch_device", "dsp_classify_signal_batch_pcm16_device", "dsp_upsample_linear_device",
        "dsp_resample_clips_device", "dsp_resample_clips_pcm16_device"}
    assert by_group["B"] >= {
        "dsp_mfcc_clips_ragged_device", "dsp_mfcc_clips_ragged_pcm16_device", "dsp_scrubjay_fused_ragged_device", "dsp_scrubjay_fused_ragged_pcm16_device",
        "dsp_classify_signal_batch_ragged_device", "dsp_classify_signal_batch_ragged_pcm16_device"}
    ids = {c.id for c in FO.CASES}
    for kind in ("512", "400", "1024", "2048"):                                  # the plans the issue names for the clip entry
        assert f"A_mfcc_clips_{kind}_f32" in ids
    for form in ("i16", "ch0", "avg"):                                          # mono, stereo channel 0, stereo average
        assert f"A_mfcc_clips_512_{form}" in ids


def test_declared_positions():
    seen = 0
    for c in FO.CASES:
        for lay, aligned in c.layouts:
            elem_bytes = 4 if "width" in lay else FO.ELEM_BYTES[c.elem]          # (matrices and strided outputs are float32)
            if "far_stride" in lay and lay["n"] in (FO.UPSAMPLE_OUT, -(-FO.RESAMPLE_IN * 160 // 441)):
                elem_bytes = 4
            FO.check_layout(lay, elem_bytes, aligned)
            if "far_stride" in lay:
                assert lay["far_stride"] % FO.ALIGN == 0 and lay["compact_stride"] % FO.ALIGN == 0 and lay["far_stride"] % 2 == 0
                assert lay["far_stride"] >= lay["n"] and (lay["k"] - 1) * lay["far_stride"] + lay["n"] + FO.OUT0 + FO.PAD <= FO.payload_elements(elem_bytes)
            if "far_offsets" in lay:
                off = lay["far_offsets"]
                assert all(a < b for a, b in zip(off, off[1:])) and max(b - a for a, b in zip(off, off[1:])) < FO.B31      # a clip holds fewer than 2^31 samples
            seen += 1
    assert seen >= len(FO.CASES)


def test_the_layouts_at_the_sizes_the_cases_use():
    lay = FO.uniform_layout(16000, 4, "straddle")
    assert lay["far"] == [0, FO.B31 - 4000, FO.B32 - 8000]                       # [2^31 - n/4, 2^31 + 3n/4) and [2^32 - n/2, 2^32 + n/2)
    lay = FO.uniform_layout(16000, 8, "straddle")
    assert lay["far"][2] == FO.B31 - 8000 and lay["far"][2] * 8 > 1 << 34 - 1
    lay = FO.ragged_layout(FO.CLIP, 4)
    assert lay["probes"] == [0, 2, 4, 6] and len(lay["far_offsets"]) == 8
    assert abs(FO.B31 - lay["far"][1] - FO.CLIP // 4) < FO.ALIGN and abs(FO.B32 - lay["far"][2] - FO.CLIP // 2) < FO.ALIGN
    lay = FO.rows_layout(400, 3)
    assert lay["far_rows"][1] * 400 < FO.B31 < (lay["far_rows"][1] + 2) * 400   # a frame of 400 straddles 2^31 itself
    assert (lay["far_rows"][1] + 1) * 400 < FO.B31 < (lay["far_rows"][1] + 2) * 400
    lay = FO.rows_layout(512, 3)
    assert lay["far_rows"][1] + 2 == (1 << 22) and lay["total_rows"] > (1 << 22) + 64
    assert FO.GUARD_BYTES == FO.B31 * max(FO.ELEM_BYTES.values()) and FO.PAYLOAD_BYTES >= (FO.B32 + 1) * 4 and FO.PAYLOAD_BYTES >= (FO.B31 + 1) * 8
