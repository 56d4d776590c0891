"""What tests/test_verify_cpu.py and tests/test_gpu_verify.py share: the fixture trials and the synthetic cases of the shape sweep, each
with its float64 reference and its float32 model (tests/verify_ref.py) computed once per session and never changed, and the rule for
`best`."""
import numpy as np

from tests import enroll_ref as E
from tests import verify_ref as V
from tests.enroll_util import fixture

SWEEP_LENS = [1, 2, 63, 64, 65, 255, 256, 257, 700]
SWEEP_LEAD = 3                                      # rows of no clip in front of the first
SWEEP_SPEAKERS = [1, 3, V.SPEAKER_TILE, V.SPEAKER_TILE + 1, 2 * V.SPEAKER_TILE + 1]
SWEEP_KD = [(k, d) for k in (1, 5, 32, 64) for d in (1, 13, 16)]
SHIFT_SIGMA = 0.6                                   # the synthetic speakers' shift: far enough apart for `best` to be decided (checked on the CPU)
_cache = {}


def offsets(lens, lead=0):
    return np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.int64)


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return case


def fixture_case(golden):
    """the twelve clips of speaker_enroll_ref.npz against its twelve relevance-MAP speakers (float32), with sklearn's scores"""
    if "fixture" not in _cache:
        z, ubm, feats = fixture(golden)
        means = z["relevance__means"].astype(np.float32)
        fo = z["frame_offsets"].astype(np.int64)
        g = golden("speaker_verify_ref.npz")
        _cache["fixture"] = _freeze({"ubm": ubm, "feats": feats, "fo": fo, "means": means, "want": V.verify(feats, fo, ubm, means),
                                     "model": V.verify(feats, fo, ubm, means, np.float32),
                                     "sklearn": {"ll_ubm": g["ubm_score"], "ll_target": g["target_score"], "llr": g["target_score"] - g["ubm_score"][:, None]}})
    return _cache["fixture"]


def sweep_case(k, d):
    """a random UBM (one component at the 1e-6 variance floor), 2 T + 1 speakers enrolled by the restatement (float32 means) from 300
    rows each of a shifted draw, and nine clips of the edge lengths, clip i new rows of speaker i's draw, 3 rows of no clip in front"""
    if (k, d) not in _cache:
        rng = np.random.default_rng(7000 + 100 * k + d)
        ubm = E.random_ubm(rng, k, d)
        n_spk = SWEEP_SPEAKERS[-1]
        floor = k == 1                                                            # (the only component is the one at the floor)
        draws = [E.draw_speaker(rng, ubm, 300 + 700, SHIFT_SIGMA, skip_floor=not floor) for _ in range(n_spk)]
        means = np.stack([E.enroll(x[:300], ubm)["means"] for x in draws]).astype(np.float32)
        clips = [draws[i][300:300 + n] for i, n in enumerate(SWEEP_LENS)]
        feats = np.concatenate([np.full((SWEEP_LEAD, d), 77.0, np.float32)] + clips)
        fo = offsets(SWEEP_LENS, SWEEP_LEAD)
        _cache[(k, d)] = _freeze({"ubm": ubm, "feats": feats, "fo": fo, "means": means, "want": V.verify(feats, fo, ubm, means),
                                  "model": V.verify(feats, fo, ubm, means, np.float32)})
    return _cache[(k, d)]


def subset(ref, n_spk):
    """the outputs of verify() for the first n_spk speakers of the call it was computed for"""
    out = {"llr": ref["llr"][:, :n_spk], "ll_ubm": ref["ll_ubm"], "ll_target": ref["ll_target"][:, :n_spk]}
    out["best"] = np.argmax(out["llr"], axis=1).astype(np.int32)
    out["best_llr"] = out["llr"][np.arange(out["llr"].shape[0]), out["best"]]
    return out


def decided(want_llr, gate):
    """clips whose float64 runner-up lies more than 2 gate below the maximum (a single speaker is always decided)"""
    if want_llr.shape[1] == 1:
        return np.ones(want_llr.shape[0], bool)
    top = np.sort(want_llr, axis=1)
    return top[:, -1] - top[:, -2] > 2.0 * gate


def check_best(best, want_llr, gate):
    """the rule for `best`: within 2 gate of the float64 maximum; the float64 argmax itself wherever that is decided -> decided clips"""
    rows = np.arange(want_llr.shape[0])
    assert best.min() >= 0 and best.max() < want_llr.shape[1]
    assert np.all(want_llr[rows, best] >= want_llr.max(axis=1) - 2.0 * gate)
    sure = decided(want_llr, gate)
    assert np.array_equal(best[sure], np.argmax(want_llr, axis=1)[sure])
    return sure
