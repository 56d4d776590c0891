"""No GPU: the table of tests/stream_order.py against include/dsp_amd.h.  Every dsp_*_device entry point the header declares has a
case (or a named exemption with its reason), every name a case declares exists in the header, and every entry a case marks as
waiting is documented to wait: the comment block in front of its declaration says "waits".  An entry point added later without a
case fails here."""
import os
import re

from tests import stream_order as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"\bdsp_\w+_device(?:_f64|_cfg)?\b")


def _header():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        return f.read()


def _declared(text):
    """the device entry points the header declares: names in front of a parameter list, outside comments"""
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    return {m.group(0): m.start() for m in re.finditer(NAME.pattern + r"(?=\()", code)}


def _block_before(text, at, name):
    """the comment block of a declaration: the last comment in front of it that starts a line and names the entry (a section's
    declarations follow its block, with one-line remarks on their neighbours in between); failing that, the last such comment"""
    blocks = [m.group(0) for m in re.finditer(r"^/\*.*?\*/", text[:at], flags=re.S | re.M)]
    naming = [b for b in blocks if re.search(rf"\b{name}\b", b)]
    return (naming or blocks or [""])[-1]


def test_every_device_entry_has_a_case():
    declared = _declared(_header())
    assert len(declared) >= 72                       # the count when the table was written: the parse still finds them
    covered = SO.covered()
    assert not set(covered) & set(SO.EXEMPT), "an exempt entry needs no case"
    missing = sorted(set(declared) - set(covered) - set(SO.EXEMPT))
    assert not missing, f"device entry points without a stream-order case: {missing}"
    for name, reason in SO.EXEMPT.items():
        assert name in declared and isinstance(reason, str) and reason.strip(), name


def test_every_name_in_the_table_is_declared():
    declared = _declared(_header())
    for c in SO.CASES:
        assert c.names, c.id
        for name in c.names:
            assert NAME.fullmatch(name) and name in declared, (c.id, name)
        assert set(c.waits) <= set(c.names), c.id
    ids = [c.id for c in SO.CASES]
    assert len(ids) == len(set(ids))


def test_every_name_mentioned_in_comments_is_declared_or_known():
    """the pattern also runs over the comments: a name that only a comment carries would be an entry the header promises nowhere"""
    text = _header()
    assert set(NAME.findall(text)) == set(_declared(text))


def test_waits_are_documented():
    text = _header()
    declared = _declared(text)
    waiting = {name for c in SO.CASES for name in c.waits}
    for name in sorted(waiting):
        assert "waits" in _block_before(text, declared[name], name), f"{name} is marked `waits`, but the comment in front of its declaration does not say so"
    for c in SO.CASES:                               # an entry waits in every case or in none
        for name in c.names:
            assert (name in c.waits) == (name in waiting), (c.id, name)


def test_the_chains_of_the_issue_are_in_the_table():
    chains = {c.id: c.names for c in SO.CASES if c.id.startswith("chain_")}
    assert len(chains) == 6
    assert chains["chain_vad_power_decide_kept_select"] == ("dsp_vad_frame_power_ragged_device", "dsp_vad_decide_ragged_device",
                                                           "dsp_rows_kept_offsets_device", "dsp_rows_select_ragged_device")
    assert chains["chain_cmvn_enroll_verify_snorm_calibrate_trials"][0] == "dsp_cmvn_ragged_device"
    assert chains["chain_cmvn_enroll_verify_snorm_calibrate_trials"][-1] == "dsp_trials_evaluate_device"
