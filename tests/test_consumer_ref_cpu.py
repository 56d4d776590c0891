"""CPU: pin the numpy references of tests/consumer_ref.py -- the stop net within 2e-5 of the oracle (its sequential float32 layer-1
sum against the reference's exact one), the speaker GMM exactly -- on the golden models and on seeded random ones, and the
references' own window rule, tile rule and domain checks."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import consumer_ref as R

F32 = np.float32


def _gmms(golden):
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return s, t, u


def test_stop_reference_on_golden_model(golden):
    m, g = dict(golden("stop_model.npz")), golden("stop_ref.npz")
    net = R.StopNet(m)
    got = np.array([net.prob_feats(f) for f in g["feats"]], F32)
    assert np.abs(got - g["feats_prob"]).max() <= 2e-5
    # the reference's clips through the oracle's MFCC: the matrix form (frame-major, clamped, zero padded) against stop_features
    for i in range(7):
        mf = O.compute_mfcc((g[f"clip{i}__pcm"] / F32(32768.0)).astype(F32), 500)
        p, bound = net.prob(mf)
        assert abs(p - O.stop_predict(m, O.stop_features(m, mf))) <= 2e-5, i
        assert p == net.prob_feats(O.stop_features(m, mf)), i          # both exact layer-1 sums: the same float32
        assert 0.0 < bound < 1e-4


@pytest.mark.parametrize("case", range(10))
def test_stop_reference_on_random_models(case):
    rng = np.random.default_rng(700 + case)
    n_coef = [1, 13, 20][case % 3]
    max_frames = [1, 7, 16, 17, 98, 40, 3, 64, 23, 120][case]
    units = (int(rng.choice([1, 2, 3, 4, 5, 16])),) + tuple(int(u) for u in rng.integers(1, 17, 2)) + (1,)
    shape = R.stop_data_shape(rng, n_coef)
    m = R.random_stop_model(rng, n_coef, max_frames, units, *shape)
    ts = [0, 1, max(1, max_frames - 1), max_frames, max_frames + 5] * 3
    mats = [R.stop_rows(rng, shape, t) for t in ts]
    m = R.fit_biases(rng, m, mats)
    net = R.StopNet(m)
    got = np.array([net.prob(x)[0] for x in mats], F32)
    want = np.array([O.stop_predict(m, O.stop_features(m, x)) for x in mats], F32)
    assert np.abs(got - want).max() <= 2e-5, (case, units, np.abs(got - want).max())
    assert np.mean((got >= 0.01) & (got <= 0.99)) >= 1 / 3, got


def test_stop_scan_reference_is_the_net_per_window():
    rng = np.random.default_rng(5)
    m = R.fit_biases(rng, R.random_stop_model(rng, 3, 9, (2, 2, 2, 1)), [rng.standard_normal((9, 3)).astype(F32) for _ in range(8)])
    net = R.StopNet(m)
    mf = rng.standard_normal((60, 3)).astype(F32)
    fo = [4, 4, 10, 11, 40, 60]
    p, _ = R.stop_scan(net, mf, fo, 6, 4)
    want = [net.prob(mf[s:s + n])[0] for (_r, s, n) in R.scan_windows(fo, 6, 4)]
    assert p.tolist() == want and len(want) == 1 + 1 + 1 + 6 + 4


def test_window_rule_matches_the_planner():
    import dsp_amd
    rows = [0, 97, 98, 107, 1, 1000, 5]
    fo = np.concatenate([[3], 3 + np.cumsum(rows)])
    for wf, hop in ((98, 10), (1, 1), (98, 400), (5, 3)):
        wins = R.scan_windows(fo, wf, hop)
        wo = dsp_amd.scan_window_offsets(fo, wf, hop)
        assert np.bincount([r for r, _s, _n in wins], minlength=len(rows)).tolist() == np.diff(wo).tolist()
        for r, s, n in wins:
            assert fo[r] <= s and s + n <= fo[r + 1] and (n == wf or (n == rows[r] and (s - fo[r]) == 0))


def test_scan_tile_rule():
    """(n_coef, max_frames, units[0], window, hop) -> windows per block, the kernel's rule restated (consumer_kernels.hip)"""
    table = {(13, 500, 4, 98, 10): 64, (13, 500, 4, 98, 18): 64, (13, 500, 4, 98, 19): 16, (13, 500, 4, 98, 77): 16,
             (13, 500, 4, 98, 78): 4, (13, 500, 4, 98, 387): 4, (13, 500, 4, 98, 388): 1, (13, 500, 4, 600, 12): 64,
             (13, 500, 4, 600, 13): 16, (13, 500, 4, 600, 254): 1, (13, 500, 16, 1, 1): 64, (13, 1260, 1, 2000, 1): 1,
             (13, 1261, 1, 2000, 1): 0, (13, 1261, 1, 1260, 1): 1, (20, 1260, 1, 820, 1): 0, (20, 1260, 1, 819, 1): 1}
    for k, tw in table.items():
        assert R.stop_scan_tile(*k) == tw, k


def test_speaker_reference_on_golden(golden):
    s, t, u = _gmms(golden)
    assert np.array_equal(R.q6(s["q6_in"]), s["q6_out"].astype(np.int64))
    for i in range(4):
        mf = s[f"clip{i}__mfcc"]
        lt, lu = R.speaker_rows(t, u, mf)
        assert np.array_equal(lt, s[f"clip{i}__ll_target"]) and np.array_equal(lu, s[f"clip{i}__ll_ubm"])
        mean, label = R.speaker_means(t, u, mf, [0, mf.shape[0]])
        assert int(mean[0]) == int(s[f"clip{i}__llr_mean"]) == O.speaker_llr_mean(t, u, mf)
        assert int(label[0]) == int(s[f"clip{i}__label"]) == O.classify_speaker(t, u, mf)
    mean, label = R.speaker_means(t, u, s["synth__mfcc"], [0, 200])
    assert int(mean[0]) == int(s["synth__llr_mean"]) and int(label[0]) == int(s["synth__label"]) == 1
    # the four clips back to back as windows of 98 rows every 98
    mf = np.concatenate([s[f"clip{i}__mfcc"] for i in range(4)])
    mean, label = R.speaker_scan(t, u, mf, [0, mf.shape[0]], 98, 98)
    assert mean.tolist() == [int(s[f"clip{i}__llr_mean"]) for i in range(4)]


@pytest.mark.parametrize("k", [1, 2, 31, 64])
@pytest.mark.parametrize("d", [1, 7, 13, 16])
def test_speaker_reference_on_random_gmms(k, d):
    rng = np.random.default_rng(k * 100 + d)
    t, u = R.random_gmm(rng, k, d), R.random_gmm(rng, k, d)
    mf = R.speaker_inputs(rng, 150, d)
    mf[0, :] = R.Q6_EDGES[np.arange(d) % R.Q6_EDGES.size]
    xq = R.q6(mf)
    assert np.array_equal(xq, O.float_to_q6(mf).astype(np.int64))
    lt, lu = R.speaker_rows(t, u, mf)
    assert lt.tolist() == [O.gmm_log_likelihood(t, x.astype(np.int16)) for x in xq]
    assert lu.tolist() == [O.gmm_log_likelihood(u, x.astype(np.int16)) for x in xq]
    fo = [0, 1, 64, 65, 150]
    mean, label = R.speaker_means(t, u, mf, fo)
    assert mean.tolist() == [O.speaker_llr_mean(t, u, mf[a:b]) for a, b in zip(fo[:-1], fo[1:])]
    assert label.tolist() == [O.classify_speaker(t, u, mf[a:b]) for a, b in zip(fo[:-1], fo[1:])]


def test_q6_edges():
    x = np.array([32767.5, 32768.0, -32768.0, -32769.0, 65535.0, -0.99, -0.0, 2.0 ** 31 - 256], np.float64) / 64.0
    assert R.q6(x).tolist() == [32767, -32768, -32768, 32767, -1, 0, 0, -256]
    assert np.signbit(np.float32(R.Q6_EDGES[9])) and R.q6(R.Q6_EDGES).tolist() == O.float_to_q6(R.Q6_EDGES).astype(np.int64).tolist()


def test_references_refuse_their_domain():
    with pytest.raises(AssertionError, match="2\\^31"):
        R.q6(np.array([2.0 ** 31 / 64.0], np.float32))
    with pytest.raises(AssertionError, match="2\\^31"):
        R.q6(np.array([np.nan], np.float32))
    g = {"means": np.full((1, 16), 127, np.int8), "inv_covs": np.full((1, 16), 2 ** 31 - 1, np.int32), "log_consts": np.zeros(1, np.int16)}
    with pytest.raises(AssertionError, match="int64"):
        R.gmm_ll(g, np.full((1, 16), -32768, np.int64))
    R.gmm_ll(g, np.full((1, 16), 127, np.int64))              # the same model on inputs that keep it in range
