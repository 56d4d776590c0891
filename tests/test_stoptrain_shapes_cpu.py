"""CPU: what the stop-net trainer's cases D .. H (tests/stoptrain_ref.py case(); tests/test_gpu_stoptrain_shapes.py trains them on the
GPU) can see that A, B and C cannot.  Three mistakes of the kind the kernels' index arithmetic could hold are planted into the float64
restatement (stoptrain_ref.DEFECTS, train_run(defect=)):

  w3_stride    layer 3's kernel read with stride u2 in place of u3
  chunk_row    the first row of a 256-row validation / prob chunk behind the first replaced by the row in front of it
  padded_down  a wrong padded layer-1 width: rounded down to a power of two, the kernel of the units from there on read as 0.  (Reading
               every unit j >= 4 as 0 would change case B, whose 16 units are no padding question; rounding down is the same class of
               mistake and leaves u1 = 4, 8 and 16 alone.)

Each leaves every run of A, B and C exactly as it was, and moves at least one of D .. H by more than 1000 times that case's allowance.
The cases' structure -- which padded width, with or without padded lanes, which 256-row edges -- is asserted here from the reference
side as well.  No kernel runs here."""
import numpy as np
import pytest

from tests import stoptrain_ref as R

FIELDS = ("history", "params", "prob")


def _moved(name: str, defect: str) -> float:
    """the largest relative difference the defect makes in any run of the case"""
    c = R.case_reference(name)
    worst = 0.0
    for run, ref in zip(c["runs"], c["numpy"]):
        got = R.train_run(c["z"], c["labels"], c["n_coef"], c["max_frames"], c["units"], run, defect=defect)
        if not np.array_equal(np.isnan(got["history"]), np.isnan(ref["history"])):     # it stops at another epoch
            return np.inf
        worst = max([worst] + [R.relative(got[k], ref[k]) for k in FIELDS])
    return worst


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect(defect):
    for name in R.CASES_OLD:
        assert _moved(name, defect) == 0.0, name                                   # equal arrays: the old cases cannot see it
    ratios = {name: _moved(name, defect) / R.case_reference(name)["allow"] for name in R.CASES_NEW}
    print(f"{defect}: difference / allowance " + ", ".join(f"{n} {r:.1e}" for n, r in ratios.items()))
    seen = {"w3_stride": ("D", "F", "G", "H"), "chunk_row": ("D",), "padded_down": ("D", "F")}[defect]
    for name in R.CASES_NEW:
        assert (ratios[name] > 1000.0) == (name in seen), (name, ratios[name])     # caught where the case's shape says so, invisible elsewhere


def test_structure():
    """every padded layer-1 width is reached with and without padded lanes; the 256-row edges, the F_used edges and the unequal widths
    are where the cases' table says"""
    want = {"A": 4, "B": 16, "C": 4, "D": 8, "E": 4, "F": 16, "G": 4, "H": 8}
    forms = set()
    for name, padded in want.items():
        c = R.case_reference(name)
        u1, u2, u3, u4 = c["units"]
        assert R.padded_units(u1) == padded and u4 == 1
        forms.add((padded, u1 < padded))
        if name in R.CASES_OLD:
            assert u2 == u3
    assert forms == {(p, lanes) for p in (4, 8, 16) for lanes in (False, True)}
    assert [R.padded_units(u) for u in range(1, 17)] == [4] * 4 + [8] * 4 + [16] * 8
    frames = {name: np.diff(R.case_reference(name)["frame_offsets"]) for name in want}
    f_used = {name: R.case_reference(name)["z"].shape[1] for name in want}
    d = R.case_reference("D")
    assert d["units"] == (7, 3, 5, 1) and d["train_rows"].size > 256 and d["val_rows"].size > 256 and d["labels"].size > 512
    assert [r["batch_size"] for r in d["runs"]] == [256, 37, 33, 1, 32, 32] and max(r["epochs"] for r in d["runs"]) <= 6
    assert d["train_rows"].size % 256 == 44 and d["train_rows"].size % 37 == 4 and 37 % 32 == 5
    assert frames["D"].min() < d["max_frames"] < frames["D"].max() and f_used["D"] == 45
    assert R.case_reference("E")["units"] == (1, 1, 1, 1) and f_used["E"] == 12 < 64
    assert f_used["F"] == 280 and 0 < f_used["F"] % 256 < 64 and R.case_reference("F")["units"][1] == 16 != R.case_reference("F")["units"][2]
    g = R.case_reference("G")
    assert f_used["G"] == 256 and g["units"][1] > g["units"][0]
    h = R.case_reference("H")
    assert frames["H"].max() == 8 < h["max_frames"] and f_used["H"] == 24 and h["units"][2] == 1
    for name in ("E", "F", "G", "H"):
        c = R.case_reference(name)
        runs, n_train = c["runs"], c["train_rows"].size
        assert len(runs) == 4 and max(runs[0].get("dropout", R.HYPER["dropout"])) > 0 and runs[1]["dropout"] == R.OFF
        assert runs[2]["batch_size"] % (32 // R.padded_units(c["units"][0])) != 0 and runs[3]["batch_size"] >= n_train


def test_patience_zero_and_restore_best():
    """case D's patience-0 pair in the restatement: it stops early, one epoch behind its best, so that restore_best decides the weights
    that come back -- the two runs share their history and differ in params and prob by far more than the allowance"""
    d = R.case_reference("D")
    best, last = d["numpy"][4], d["numpy"][5]
    assert d["runs"][4]["patience"] == 0 and d["runs"][4]["restore_best"] and not d["runs"][5]["restore_best"]
    assert {k: v for k, v in d["runs"][4].items() if k not in ("restore_best", "train_rows", "val_rows")} == \
           {k: v for k, v in d["runs"][5].items() if k not in ("restore_best", "train_rows", "val_rows")}
    for r in (best, last):
        assert r["status"] == R.CONVERGED_EARLY and r["n_epochs"] < d["runs"][4]["epochs"] and r["best_epoch"] == r["n_epochs"] - 2
    assert np.array_equal(best["history"], last["history"], equal_nan=True)
    moved = R.relative(best["params"], last["params"])
    print(f"restore_best on / off: params differ by {moved:.2e} relative, {moved / d['allow']:.1e} allowances")
    assert moved > 1000.0 * d["allow"] and R.relative(best["prob"], last["prob"]) > 1000.0 * d["allow"]
    assert not d["runs"][1]["restore_best"] and d["numpy"][1]["status"] == R.MAX_EPOCHS
