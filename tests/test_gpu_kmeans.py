"""GPU: the k-means start of UBM training (dsp_kmeans_*; UbmTrainer.kmeans_seed, .kmeans, .fit(init="kmeans")) against the float64
restatement of its definitions (tests/kmeans_ref.py) and against sklearn's recorded answers (tests/golden/kmeans_ref.npz).

Labels: a row whose float64 relative margin (s_2nd - s_1st) / s_2nd exceeds 2 (d + 3) 2^-24, the rounding bound of a d-term float32 sum of
squares, owes the float64 label; any other row the best or the second best.  Sums: the gate of tests/test_gpu_ubm.py -- a GPU value may
deviate from float64 by GATE_FACTOR = 8 times what the restatement's own float32 model deviates on the same inputs, floored at
8 * 2^-23 * max | value |, variances relatively -- always against float64 statistics OF THE GPU'S LABELS.  Seeding: the validity rule of
tests/kmeans_ref.py seeding_is_valid, which does not ask float32 to reproduce a discrete draw.  Then what must hold bit for bit."""
import numpy as np
import pytest

from tests import kmeans_ref as K
from tests import ubm_ref as U
from tests.kmeans_util import CASES, fixture, fixture_lloyd

pytestmark = pytest.mark.gpu
GROUP_ROWS = U.CHUNK_ROWS * U.GROUP_CHUNKS
START_KEYS = ("weights", "means", "variances")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _cuda(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _mixture(rng, n, k, d):
    """rows around k centres, and a start: k of the rows, each moved by a fraction of the spread"""
    x = (rng.normal(0.0, 2.0, (k, d))[rng.integers(0, k, n)] + rng.normal(0.0, 0.7, (n, d))).astype(np.float32)
    start = x[rng.choice(n, k, replace=False)].astype(np.float64) + 0.05 * rng.normal(size=(k, d))
    return x, start


def _step_case(k, d, n):
    """the first seed at which no row lies inside twice the rounding bound, neither of the first labelling -- the centres after one step are
    then owed exactly the float64 labels' -- nor of the labelling against those centres (both asserted by the caller, on the inputs)"""
    for seed in range(50):
        x, start = _mixture(np.random.default_rng(100000 * seed + 1000 * k + 10 * d + n % 7), n, k, d)
        labels0, s0 = K.label_rows(x, start)
        if K.margins(s0).min() > 2.0 * K.rounding_bound(d) and K.margins(K.sq_dists(x, _after_one_step(x, start, labels0, np.float64))).min() > 2.0 * K.rounding_bound(d):
            return x, start
    raise AssertionError("no seed keeps every row outside the margin")


def _as_fit(res):
    """a k-means result in the shape tests/ubm_ref.py's gates take: the GMM start, its log_consts, and the inertia where the lower bounds go"""
    return {"weights": res["weights"], "means": res["means"], "variances": res["variances"], "log_consts": U.log_consts(res["weights"], res["variances"]),
            "lower_bounds": np.array([res["inertia"]])}


def _check_sums(got, want, model, what):
    gates, dev = U.gates(_as_fit(model), _as_fit(want)), U.deviations(_as_fit(got), _as_fit(want))
    print(f"\nkmeans {what}: " + ", ".join(f"{key} {dev[key]:.2e} / {gates[key]:.2e}" for key in gates) + "  (GPU vs float64 / gate; lower_bounds = inertia)")
    for key in gates:
        assert np.isfinite(_as_fit(got)[key]).all() and dev[key] <= gates[key], (what, key, dev[key], gates[key])


def _check_centres(got, want, model, what):
    gate = max(U.GATE_FACTOR * float(np.abs(model - want).max()), 8.0 * 2.0 ** -23 * float(np.abs(want).max()))
    dev = float(np.abs(got - want).max())
    print(f"\nkmeans {what}: centres {dev:.2e} / {gate:.2e}")
    assert np.isfinite(got).all() and dev <= gate, (what, dev, gate)


def _check_labels(x, centres, labels, what, share=1e-3):
    """labels against `centres` (float64): outside the rounding bound the float64 label, inside it the best or the second best; at most
    `share` of the rows are inside, so that the test cannot pass by excusing rows"""
    d = x.shape[1]
    s = K.sq_dists(x, centres)
    inside = K.margins(s) <= K.rounding_bound(d)
    assert inside.mean() <= share, (what, float(inside.mean()))
    best = np.argmin(s, axis=1)
    assert np.array_equal(labels[~inside], best[~inside]), what
    if inside.any():
        order = np.argsort(s[inside], axis=1, kind="stable")[:, :2]
        assert np.all((labels[inside, None] == order).any(axis=1)), what
    return int(inside.sum())


def _one_step(k, d, n):
    x, start = _step_case(k, d, n)
    labels0, s0 = K.label_rows(x, start)
    assert K.margins(s0).min() > 2.0 * K.rounding_bound(d)          # on the inputs: every first label is owed
    inside = K.margins(K.sq_dists(x, _after_one_step(x, start, labels0, np.float64))) <= K.rounding_bound(d)
    assert inside.mean() <= 1e-3                                     # and at most 0.1 % of the second ones could be excused
    return x, start, labels0


def _after_one_step(x, start, labels0, dtype):
    N, F, _ = K.labelled_statistics(x, start, labels0, dtype)
    c = start.astype(dtype).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(N[:, None] > 0, c + F / N[:, None], start)


def _final_of(x, got, dtype):
    """the statistics of the GPU's own final labels against its own final centres, in `dtype`"""
    labels = got["labels"].cpu().numpy()
    out = K.gmm_start(x, got["centres"], labels, 1e-6, dtype)
    out["inertia"] = K.inertia_of(K.sq_dists(x, got["centres"], dtype), labels, dtype)
    return out


ROWS = {"n_eq_k": None, "chunk-1": U.CHUNK_ROWS - 1, "chunk": U.CHUNK_ROWS, "chunk+1": U.CHUNK_ROWS + 1, "group+1": GROUP_ROWS + 1, "6000": 6000}


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("d", [1, 13, 16])
@pytest.mark.parametrize("k", [1, 5, 32, 64])
def test_one_lloyd_step_on_the_edges_of_the_tree(torch_cuda, k, d, rows):
    """max_iter = 1 from given centres for every k x d on row counts k, C - 1, C, C + 1 (C = rows per chunk), one row more than a group,
    and 6000: the centres after the step, then labels, counts, inertia and GMM start of the pass behind it"""
    import dsp_amd
    n = max(ROWS[rows] or k, k)
    x, start, labels0 = _one_step(k, d, n)
    got = dsp_amd.UbmTrainer(k, d).kmeans(_cuda(torch_cuda, x), start, max_iter=1, tol=0.0, want_labels=True)
    what = f"k {k} d {d} n {n}"
    assert got["n_iter"] == 1 and got["stop"] in ("max_iter", "tol")
    _check_centres(got["centres"], _after_one_step(x, start, labels0, np.float64), _after_one_step(x, start, labels0, np.float32), what)
    labels = got["labels"].cpu().numpy()
    assert labels.dtype == np.int32 and labels.shape == (n,)
    _check_labels(x, got["centres"], labels, what)
    assert np.array_equal(got["counts"], np.bincount(labels, minlength=k)) and got["n_empty"] == int((got["counts"] == 0).sum())
    _check_sums(got, _final_of(x, got, np.float64), _final_of(x, got, np.float32), what)


@pytest.mark.parametrize("d", range(1, 17))
def test_every_d_of_the_dispatch(torch_cuda, d):
    """every d the kernels are instantiated for, at k = 5 on one chunk and one row: one Lloyd step, a seeding, and twice the same bits"""
    import dsp_amd
    k, n = 5, U.CHUNK_ROWS + 1
    x, start, labels0 = _one_step(k, d, n)
    xd = _cuda(torch_cuda, x)
    tr = dsp_amd.UbmTrainer(k, d)
    got = tr.kmeans(xd, start, max_iter=1, tol=0.0, want_labels=True)
    _check_centres(got["centres"], _after_one_step(x, start, labels0, np.float64), _after_one_step(x, start, labels0, np.float32), f"d {d}")
    _check_labels(x, got["centres"], got["labels"].cpu().numpy(), f"d {d}")
    _check_sums(got, _final_of(x, got, np.float64), _final_of(x, got, np.float32), f"d {d}")
    again = tr.kmeans(xd, start, max_iter=1, tol=0.0, want_labels=True)
    assert all(np.array_equal(again[key], got[key]) for key in ("centres", "counts") + START_KEYS) and again["inertia"] == got["inertia"]
    picked = tr.kmeans_seed(xd, 11)
    assert K.seeding_is_valid(x, picked, 11) is None and np.array_equal(tr.kmeans_seed(xd, 11), picked)


@pytest.mark.parametrize("tag", CASES)
def test_fixture_trajectories_are_sklearns(torch_cuda, golden, tag):
    """sklearn's n_iter, its stop reason and every label; centres and GMM start within the gate of sklearn's"""
    import dsp_amd
    z, x, sk = fixture(golden, tag)
    ref64, ref32 = fixture_lloyd(golden, tag), fixture_lloyd(golden, tag, np.float32)
    k, d = sk["centres"].shape
    got = dsp_amd.UbmTrainer(k, d).kmeans(_cuda(torch_cuda, x), x.astype(np.float64)[sk["start"]], max_iter=300, tol=float(z["tol"]),
                                          reg_covar=float(z["reg_covar"]), want_labels=True)
    assert got["n_iter"] == int(sk["n_iter"]) and got["stop"] == str(sk["stop"]) and got["n_empty"] == 0
    assert np.array_equal(got["labels"].cpu().numpy(), sk["labels"]) and np.array_equal(got["counts"], np.bincount(sk["labels"], minlength=k))
    _check_centres(got["centres"], sk["centres"], ref32["centres"], f"fixture {tag}")
    want = dict({key: sk[key] for key in START_KEYS}, inertia=float(sk["inertia"]))
    # (the gate is the float32 model's deviation from the float64 restatement, which is sklearn to 4e-14)
    gates, dev = U.gates(_as_fit(ref32), _as_fit(ref64)), U.deviations(_as_fit(got), _as_fit(want))
    print(f"\nkmeans fixture {tag}: " + ", ".join(f"{key} {dev[key]:.2e} / {gates[key]:.2e}" for key in gates) + "  (GPU vs sklearn / gate)")
    for key in gates:
        assert dev[key] <= gates[key], (tag, key, dev[key], gates[key])


def test_an_empty_cluster_keeps_its_centre(torch_cuda):
    """one start centre at 1e3: n_empty = 1, that centre comes back as it went in, its GMM component is the one no row visits (mean 0,
    variance reg_covar, a weight of about 1e-15 / n); the other clusters are the restatement's"""
    import dsp_amd
    k, d, n = 5, 13, 2000
    x, start = _mixture(np.random.default_rng(77), n, k, d)
    start[2] = 1e3
    want, model = K.lloyd(x, start, 4, 0.0, 1e-5), K.lloyd(x, start, 4, 0.0, 1e-5, np.float32)
    assert want["n_empty"] == 1 and want["counts"][2] == 0 and np.array_equal(want["labels"], model["labels"]) and want["n_iter"] == model["n_iter"]
    got = dsp_amd.UbmTrainer(k, d).kmeans(_cuda(torch_cuda, x), start, max_iter=4, tol=0.0, reg_covar=1e-5, want_labels=True)
    assert got["n_empty"] == 1 and got["counts"][2] == 0 and np.all(got["centres"][2] == 1e3) and got["n_iter"] == want["n_iter"] and got["stop"] == want["stop"]
    assert np.all(got["means"][2] == 0.0) and np.all(got["variances"][2] == 1e-5) and abs(got["weights"][2] / want["weights"][2] - 1.0) < 1e-6
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    _check_centres(got["centres"], want["centres"], model["centres"], "empty cluster")
    _check_sums(got, want, model, "empty cluster")


@pytest.mark.parametrize("n,k,d", [(64, 64, 3), (700, 5, 1), (1500, 8, 13), (4097, 64, 16)])
def test_seeding_is_a_valid_greedy_kmeanspp(torch_cuda, n, k, d):
    import dsp_amd
    x, _ = _mixture(np.random.default_rng(1000 * n + k), n, k, d)
    tr = dsp_amd.UbmTrainer(k, d)
    xd = _cuda(torch_cuda, x)
    for seed in (0, 42, 2 ** 64 - 1):
        rows = tr.kmeans_seed(xd, seed)
        assert rows.dtype == np.int64 and rows.shape == (k,) and rows.min() >= 0 and rows.max() < n
        assert K.seeding_is_valid(x, rows, seed) is None, (seed, K.seeding_is_valid(x, rows, seed))
    if n == k:
        assert sorted(rows.tolist()) == list(range(n))                # every row becomes a centre


def test_fewer_than_k_distinct_rows_is_a_named_error(torch_cuda):
    import dsp_amd
    k, d = 8, 13
    x, _ = _mixture(np.random.default_rng(5), 600, k, d)
    few = np.tile(x[:k - 1], (40, 1))                                  # 280 rows, 7 distinct
    tr = dsp_amd.UbmTrainer(k, d)
    with pytest.raises(dsp_amd.DspError, match="fewer than k = 8 distinct rows"):
        tr.kmeans_seed(_cuda(torch_cuda, few), 3)
    with pytest.raises(dsp_amd.DspError, match="distinct rows"):
        tr.fit(_cuda(torch_cuda, few), init="kmeans", max_iter=2)
    rows = tr.kmeans_seed(_cuda(torch_cuda, x), 3)                     # the trainer is usable afterwards
    assert K.seeding_is_valid(x, rows, 3) is None


def _whole(tr, xd, x, seed):
    """seeding, then Lloyd from the seed rows -> (rows, the k-means result with its labels)"""
    rows = tr.kmeans_seed(xd, seed)
    return rows, tr.kmeans(xd, x.astype(np.float64)[rows], max_iter=40, want_labels=True)


def _same_kmeans(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "rows")
    for key in ("centres", "counts", "inertia", "n_iter", "stop", "n_empty") + START_KEYS:
        assert np.array_equal(a[1][key], b[1][key]), (what, key)
    assert bool((a[1]["labels"] == b[1]["labels"]).all()), (what, "labels")


def test_bit_identity_across_calls_workspaces_addresses_and_trainers(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    k, d, n = 32, 13, 2 * GROUP_ROWS + 300
    x, _ = _mixture(np.random.default_rng(9), n, k, d)
    xd = _cuda(torch, x)
    tr = dsp_amd.UbmTrainer(k, d)
    kw = dict(init="kmeans", n_init=2, seed=42, max_iter=4, tol=0.0, kmeans_max_iter=40)
    first, model = _whole(tr, xd, x, 42), tr.fit(xd, **kw)
    _same_kmeans(_whole(tr, xd, x, 42), first, "the same call twice")
    big = _cuda(torch, np.concatenate([x[::-1]] * 3))
    tr.fit(big, init="kmeans", max_iter=2, kmeans_max_iter=3)          # a larger problem grows the workspace and leaves its own sums there
    _same_kmeans(_whole(tr, xd, x, 42), first, "after the workspace has grown")
    buf = torch.zeros(n * d + 8, dtype=torch.float32, device="cuda")
    moved = buf[1:1 + n * d].view(n, d)                                # 4 bytes past a 16-byte boundary
    moved.copy_(xd)
    assert moved.data_ptr() % 16 == 4 and moved.is_contiguous()
    _same_kmeans(_whole(tr, moved, x, 42), first, "rows at another address")
    other = dsp_amd.UbmTrainer(k, d)
    _same_kmeans(_whole(other, xd, x, 42), first, "another trainer")
    for who, rows in (("again", xd), ("moved", moved)):
        again = (tr if who == "again" else other).fit(rows, **kw)
        for key in ("weights", "means", "variances", "log_consts", "inv_covs", "lower_bounds", "n_iter", "converged"):
            assert np.array_equal(again[key], model[key]), (who, key)
        assert again["report"]["winner"] == model["report"]["winner"]
        for a, b in zip(again["report"]["restarts"], model["report"]["restarts"]):
            assert all(np.array_equal(a[key], b[key]) for key in a), who


def test_the_stop_is_honoured_by_the_launches_behind_it(torch_cuda, golden):
    """the tol case stops after 29 iterations while the centres still creep: the launches enqueued behind the stop (the host looks every
    32) leave them alone -- max_iter = 300 gives the bits of max_iter = 29, which one more iteration would not"""
    import dsp_amd
    z, x, sk = fixture(golden, "tol")
    ref = fixture_lloyd(golden, "tol")
    n_iter = int(sk["n_iter"])
    assert n_iter % 32 != 0 and n_iter == 29
    xd, start = _cuda(torch_cuda, x), x.astype(np.float64)[sk["start"]]
    tr = dsp_amd.UbmTrainer(5, 1)
    long_run, exact, more = (tr.kmeans(xd, start, max_iter=m, tol=tol) for m, tol in ((300, float(z["tol"])), (n_iter, 0.0), (n_iter + 1, 0.0)))
    assert long_run["n_iter"] == n_iter and long_run["stop"] == "tol" and exact["n_iter"] == n_iter and exact["stop"] == "max_iter"
    assert np.array_equal(long_run["centres"], exact["centres"]) and long_run["inertia"] == exact["inertia"]
    assert more["n_iter"] == n_iter + 1 and not np.array_equal(more["centres"], exact["centres"])
    assert np.abs(long_run["centres"] - ref["centres"]).max() < 1e-5


def test_n_init_restarts_are_the_separate_runs_and_the_best_is_kept(torch_cuda, golden):
    """n_init = 3: each restart's last lower bound is that of kmeans_seed -> kmeans -> fit(init=...) with the restart's seed, bit for bit;
    the model returned is the argmax, ties to the first; and on a drawn population it is no worse than the library's row start"""
    import dsp_amd
    torch = torch_cuda
    zz = golden("speaker_enroll_ref.npz")
    ref_ubm = {key: zz[f"ubm_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
    x = U.draw_population(np.random.default_rng(7311), ref_ubm, 20000)
    xd = _cuda(torch, x)
    tr = dsp_amd.UbmTrainer(32, 13)
    got = tr.fit(xd, init="kmeans", n_init=3, seed=42, max_iter=30)
    report = got["report"]
    assert len(report["restarts"]) == 3
    separate = []
    for r, rep in enumerate(report["restarts"]):
        rows = tr.kmeans_seed(xd, K.restart_seed(42, r))
        km = tr.kmeans(xd, x.astype(np.float64)[rows])
        fit = tr.fit(xd, init=km, max_iter=30)
        separate.append(fit)
        assert np.array_equal(rows, rep["rows"]) and K.seeding_is_valid(x, rows, K.restart_seed(42, r)) is None
        assert (km["n_iter"], km["stop"], km["n_empty"]) == (rep["kmeans_n_iter"], rep["kmeans_stop"], rep["kmeans_n_empty"])
        assert (fit["n_iter"], fit["converged"]) == (rep["em_n_iter"], rep["em_converged"]) and fit["lower_bounds"][-1] == rep["lower_bound"]
    bounds = [rep["lower_bound"] for rep in report["restarts"]]
    assert report["winner"] == int(np.argmax(bounds))                  # (argmax: the first of equals)
    for key in ("weights", "means", "variances", "log_consts", "inv_covs", "lower_bounds", "n_iter", "converged"):
        assert np.array_equal(got[key], separate[report["winner"]][key]), key
    plain = tr.fit(xd, max_iter=30)
    print(f"\nn_init 3: last lower bounds {bounds}, winner {report['winner']}; the row start's {plain['lower_bounds'][-1]}")
    assert got["lower_bounds"][-1] >= plain["lower_bounds"][-1]
    one = tr.fit(xd, init="kmeans", n_init=1, seed=42, max_iter=30)    # n_init = 1 is restart 0 alone
    assert one["report"]["winner"] == 0 and np.array_equal(one["lower_bounds"], separate[0]["lower_bounds"])


def test_one_em_iteration_from_hard_posteriors_is_the_kmeans_start(torch_cuda):
    """three clusters 1000 apart at unit noise, 700 rows (two chunks and a partial one): from the k-means centres at variance 1 every
    float32 posterior is exactly 0 or 1, so one EM iteration sums what Lloyd's final pass summed and the M-step both call gives the
    same weights, means and variances, bit for bit"""
    import dsp_amd
    k, d, n = 3, 2, 700
    which = np.arange(n) % k
    x = (1000.0 * which[:, None] + np.random.default_rng(3).normal(size=(n, d))).astype(np.float32)
    start = np.stack([x[which == i].astype(np.float64).mean(axis=0) for i in range(k)])
    xd = _cuda(torch_cuda, x)
    tr = dsp_amd.UbmTrainer(k, d)
    km = tr.kmeans(xd, start, max_iter=1, tol=0.0, reg_covar=1e-6, want_labels=True)
    assert np.array_equal(km["labels"].cpu().numpy(), which)
    em = tr.fit(xd, init={"weights": np.full(k, 1.0 / k), "means": km["centres"], "variances": np.ones((k, d))}, max_iter=1, tol=0.0, reg_covar=1e-6)
    for key in START_KEYS:
        assert np.array_equal(em[key], km[key]), key


def test_kmeans_start_then_em_is_sklearns_gaussian_mixture(torch_cuda, golden):
    """the fixture's k-means start, then 10 EM iterations, against sklearn's recorded GaussianMixture answer from its own start, within
    the gate tests/test_gpu_ubm.py's fixture test uses"""
    import dsp_amd
    z, x, sk = fixture(golden, "strict")
    k, d = sk["centres"].shape
    reg = float(z["reg_covar"])
    start64, start32 = fixture_lloyd(golden, "strict"), fixture_lloyd(golden, "strict", np.float32)
    ref64 = U.fit(x, start64, max_iter=10, tol=0.0, reg_covar=reg)
    ref32 = U.fit(x, start32, max_iter=10, tol=0.0, reg_covar=reg, dtype=np.float32)
    tr = dsp_amd.UbmTrainer(k, d)
    xd = _cuda(torch_cuda, x)
    km = tr.kmeans(xd, x.astype(np.float64)[sk["start"]], tol=float(z["tol"]), reg_covar=reg)
    got = tr.fit(xd, init=km, max_iter=10, tol=0.0, reg_covar=reg)
    assert got["n_iter"] == int(sk["em_n_iter"]) == 10
    want = U.result(sk["em_weights"], sk["em_means"], sk["em_variances"])
    want["lower_bounds"] = np.array([float(sk["em_lower_bound"])])
    gates = U.gates(dict(ref32, lower_bounds=ref32["lower_bounds"][-1:]), dict(ref64, lower_bounds=ref64["lower_bounds"][-1:]))
    dev = U.deviations(dict(got, lower_bounds=got["lower_bounds"][-1:]), want)
    print("\nkmeans start + EM: " + ", ".join(f"{key} {dev[key]:.2e} / {gates[key]:.2e}" for key in gates) + "  (GPU vs sklearn / gate)")
    for key in gates:
        assert dev[key] <= gates[key], (key, dev[key], gates[key])
