"""GPU: stop-net training (dsp_stop_train_*) at the kernel forms and row counts tests/test_gpu_stoptrain.py does not
reach, against the same float64 restatement (tests/stoptrain_ref.py), on the cases D .. H of stoptrain_ref.case():

  D  5 x 9, units 7-3-5-1, 600 clips of 3 .. 11 frames, 300 / 300: the <8> kernels with one padded lane, three unequal odd widths; the
     scaler tree's second pass, a full batch of 256, validation chunks 256 + 44, prob chunks 256 + 256 + 88; restore_best off,
     patience 0
  E  2 x 6, units 1-1-1-1, 40 clips of 2 .. 7 frames: the smallest net, F_used 12 below a wavefront
  F  4 x 70, units 12-16-9-1, 90 clips of 70 frames: the <16> kernels with four padded lanes, F_used 280 (lanes 0 .. 23 own two features)
  G  16 x 16, units 3-5-2-1, 50 clips of 16 frames: the <4> kernels with a padded lane, u2 > u1, F_used 256 exactly
  H  3 x 11, units 8-16-1-1, 60 clips of 2 .. 8 frames: the <8> kernels without padding, u3 = 1, the longest clip below max_frames

The allowance is each case's own, imported: four times the restatement's spread between the ascending and descending layer-1 sums,
floored at 1e-9 relative (asserted on the CPU by tests/test_stoptrain_cpu.py test_restatement_spread; spreads 2e-16 .. 5e-15, so the
floor holds).  That each case reaches its edge is asserted on the reference side, here and in tests/test_stoptrain_shapes_cpu.py, which
also shows what mistakes these cases catch that A, B and C cannot.  Nothing here is derived from what the GPU returns."""
import numpy as np
import pytest

from dsp_amd import lib as dl

from tests import stoptrain_ref as R
from tests import stoptrain_util as U

pytestmark = pytest.mark.gpu
CASES = R.CASES_NEW
PADDED = {"D": 8, "E": 4, "F": 16, "G": 4, "H": 8}


@pytest.fixture(scope="module")
def cases():
    """per case: the restatement's answers (computed once, left unchanged) and the device's, from ONE launch of all of its runs"""
    yield from U.trained_cases(CASES)


@pytest.mark.parametrize("name", CASES)
def test_scaler_and_rows(cases, name):
    """Scaler and standardised rows bit for bit; in D the Scaler's lanes take two rows each, in H the inputs past the longest clip have
    mean 0 and scale 1"""
    c = cases[name]
    z = U.check_scaler_and_rows(c)
    frames = np.diff(c["frame_offsets"])
    if name == "D":
        assert c["train_rows"].size == 300 > 256 and frames.min() < c["max_frames"] < frames.max()
    if name == "G":
        assert z.shape[1] == c["trainer"].f_used == 256
    if name == "F":
        assert 0 < c["trainer"].f_used % 256 < 64
    if name == "H":
        t_used = R.used_frames(c["frame_offsets"], c["max_frames"])
        assert t_used == frames.max() < c["max_frames"]
        unused = np.setdiff1d(np.arange(c["n_coef"] * c["max_frames"]), R.used_index(c["n_coef"], c["max_frames"], t_used))
        assert unused.size == c["n_coef"] * (c["max_frames"] - t_used) and (c["got_mean"][unused] == 0).all() and (c["got_scale"][unused] == 1).all()


@pytest.mark.parametrize("name", CASES)
def test_trajectories(cases, name):
    """history, params and prob within the case's allowance, the integer results exactly, behind the structure the case is there for"""
    c = cases[name]
    u1, n_train, runs = c["units"][0], c["train_rows"].size, c["runs"]
    assert R.padded_units(u1) == PADDED[name] and tuple(c["trainer"].units) == c["units"]
    if name == "D":
        assert c["val_rows"].size > 256 and c["labels"].size > 512 and runs[0]["batch_size"] == 256 <= n_train and u1 < 8
        assert runs[1]["batch_size"] == 37 and not runs[1]["restore_best"] and runs[3]["batch_size"] == 1 and runs[4]["patience"] == 0
        assert max(r["epochs"] for r in runs) <= 6
    else:
        assert len(runs) == 4 and runs[1]["dropout"] == R.OFF and max(runs[0].get("dropout", R.HYPER["dropout"])) > 0
        assert runs[2]["batch_size"] % (32 // PADDED[name]) != 0 and runs[3]["batch_size"] >= n_train
    U.check_trajectories(c)
    if name == "D":
        assert c["res"][4]["status"] == dl.STOP_TRAIN_CONVERGED_EARLY and c["res"][4]["n_epochs"] < runs[4]["epochs"]
    if name == "H":                                                  # kernel1 rows of the inputs no clip reaches: the initial draws
        t_used, u1 = R.used_frames(c["frame_offsets"], c["max_frames"]), c["units"][0]
        unused = np.setdiff1d(np.arange(c["n_coef"] * c["max_frames"]), R.used_index(c["n_coef"], c["max_frames"], t_used))
        for k, run in enumerate(runs):
            first = R.init(c["n_coef"], c["max_frames"], c["units"], run["seed"])[:c["n_coef"] * c["max_frames"] * u1].reshape(-1, u1)
            got = c["params"][k][:first.size].reshape(-1, u1)
            assert unused.size == 9 and np.array_equal(got[unused], first[unused]) and not np.array_equal(got, first)


def test_every_form_with_and_without_padding():
    """across the old and the new cases the <4>, <8> and <16> kernels each run with u1 == U1P and with u1 < U1P"""
    forms = {(R.padded_units(R.SHAPES[name][2][0]), R.SHAPES[name][2][0] < R.padded_units(R.SHAPES[name][2][0])) for name in R.CASES_OLD + R.CASES_NEW}
    assert forms == {(p, lanes) for p in (4, 8, 16) for lanes in (False, True)}


def test_restore_best(cases):
    """case D without restore_best returns the restatement's last weights; the patience-0 pair, which stops one epoch behind its best,
    differs between restore_best on and off as the restatement's does (shown first)"""
    c = cases["D"]
    ref_best, ref_last = c["numpy"][4], c["numpy"][5]
    assert ref_best["status"] == R.CONVERGED_EARLY and ref_best["n_epochs"] < c["runs"][4]["epochs"] and ref_best["best_epoch"] != ref_best["n_epochs"] - 1
    assert R.relative(ref_best["params"], ref_last["params"]) > 1000.0 * c["allow"]
    for k in (1, 5):                                                 # the runs without restore_best: the last weights
        assert not c["runs"][k]["restore_best"] and R.relative(c["params"][k], c["numpy"][k]["params"]) <= c["allow"]
    moved = R.relative(c["params"][4], c["params"][5])
    print(f"D patience 0: restore_best on / off differ by {moved:.2e} relative (the restatement: {R.relative(ref_best['params'], ref_last['params']):.2e})")
    assert moved > 1000.0 * c["allow"] and R.relative(c["params"][4], ref_best["params"]) <= c["allow"]
    assert np.array_equal(c["hist"][4], c["hist"][5], equal_nan=True)


def test_bit_identity(cases):
    """one case-D run alone, among 20 others and in the reversed launch: equal bytes of history, params, prob and result at U1P = 8"""
    c = cases["D"]
    t = c["trainer"]
    run = dict(c["runs"][1], epochs=2)
    alone = U.result_bytes(*t.train([run], c["labels"]), 0)
    others = [dict(run, seed=1000 + k, batch_size=1 + 9 * k, epochs=1 + k % 2) for k in range(20)]
    mixed = others[:10] + [run] + others[10:]
    assert U.result_bytes(*t.train(mixed, c["labels"]), 10) == alone
    assert U.result_bytes(*t.train(mixed[::-1], c["labels"]), 10) == alone


@pytest.mark.parametrize("name,k", (("D", 2), ("F", 1)))
def test_round_trip(cases, name, k):
    """a trained model of the <8> and of the <16> form through dsp_stop_model_from_training -> StopModel -> predict on the case's own
    MFCC, on a dozen rows, clips shorter and longer than max_frames among them in D"""
    c = cases[name]
    rows = list(range(0, c["labels"].size, c["labels"].size // 12))[:12]
    if name == "D":
        frames = np.diff(c["frame_offsets"])[rows]
        assert frames.min() < c["max_frames"] < frames.max()
    U.check_round_trip(c, k, rows)
