"""GPU: UBM training (dsp_ubm_*; dsp_amd.UbmTrainer, dsp_amd.quantize_gmm) against the float64 restatement of its definitions
(tests/ubm_ref.py) and against sklearn's recorded answers (tests/golden/ubm_train_ref.npz).

The gate, per output and case: a GPU value may deviate from float64 by GATE_FACTOR = 8 times what the restatement's own float32 model
deviates on the same inputs (computed here from tests/ubm_ref.py, never from the library; 8 covers another summation order and the
hardware's exp, log and division), floored at 8 * 2^-23 * max | value | where the model happens to be exact.  Variances are compared
relatively.  Then what must hold bit for bit: the same call twice, after the workspace has grown, from another device address, from another
trainer."""
import ctypes as C

import numpy as np
import pytest

from tests import consumer_ref as R
from tests import enroll_ref as E
from tests import ubm_ref as U
from tests.ubm_util import fixture, fixture_fit

pytestmark = pytest.mark.gpu
OUTPUTS = ("weights", "means", "variances", "log_consts", "inv_covs", "lower_bounds", "n_iter", "converged")
GROUP_ROWS = U.CHUNK_ROWS * U.GROUP_CHUNKS
SEED = 4        # EM on 255 rows with 64 components is ill-conditioned: two float32 summation orders can differ from float64 by amounts a factor of
                # ten apart.  Chosen from tests/ubm_ref.py alone: at this seed a second float32 model of every case of the sweep below (a
                # chunk summed as four interleaved quarters, combined in order) stays within 0.59 of the gates of the sequential one; seeds
                # 1 .. 7 otherwise reach 1.0 .. 7.9


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _cuda(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _prefix(ref, i):
    """the result of max_iter = i at tol = 0 out of a longer history"""
    out = U.result(*ref["models"][i - 1])
    out.update(lower_bounds=ref["lower_bounds"][:i], n_iter=i, converged=False)
    return out


def _check(got, want, model, what):
    gates, dev = U.gates(model, want), U.deviations(got, want)
    print(f"\nubm {what}: " + ", ".join(f"{key} {dev[key]:.2e} / {gates[key]:.2e}" for key in gates) + "  (GPU vs float64 / gate)")
    for key in gates:
        assert np.isfinite(got[key]).all() and dev[key] <= gates[key], (what, key, dev[key], gates[key])
    assert np.array_equal(got["inv_covs"], 1.0 / got["variances"]) and got["n_iter"] == want["n_iter"] and got["converged"] == want["converged"]
    return dev, gates


def _same(a, b, what):
    for key in OUTPUTS:
        assert np.array_equal(a[key], b[key]), (what, key)


def _case(k, d, n):
    """rows of a population under a random UBM with variances log-uniform in [1e-6, 4] and one component at the floor (k = 1: drawn from
    that one), and a caller's start: that UBM with its means moved by a tenth of a standard deviation"""
    rng = np.random.default_rng(100000 * SEED + 1000 * k + 10 * d + n % 7)
    ubm = E.random_ubm(rng, k, d)
    x = U.draw_population(rng, ubm, n) if k > 1 else E.draw_speaker(rng, ubm, n, 0.0, skip_floor=False)
    var = 1.0 / ubm["inv_covs"]
    w = E.weights_of(ubm)
    return x, {"weights": w / w.sum(), "means": ubm["means"] + 0.1 * np.sqrt(var) * rng.normal(size=var.shape), "variances": var}


ROWS = {"n_eq_k": None, "chunk-1": U.CHUNK_ROWS - 1, "chunk": U.CHUNK_ROWS, "chunk+1": U.CHUNK_ROWS + 1, "group+1": GROUP_ROWS + 1, "6000": 6000}


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("d", [1, 13, 16])
@pytest.mark.parametrize("k", [1, 5, 32, 64])
def test_parity_with_float64_on_the_edges_of_the_tree(torch_cuda, k, d, rows):
    """1 and 8 iterations at tol = 0 from the library's start and from a caller's, for every k x d on row counts k, C - 1, C, C + 1
    (C = rows per chunk), one row more than a group of the reduction tree, and 6000"""
    import dsp_amd
    n = ROWS[rows] or k
    x, given = _case(k, d, n)
    xd = _cuda(torch_cuda, x)
    tr = dsp_amd.UbmTrainer(k, d)
    start = tr.init_rows(xd)
    s64, s32 = U.init_rows(x, k), U.init_rows(x, k, dtype=np.float32)
    assert np.array_equal(start["means"], s64["means"]) and np.array_equal(start["weights"], s64["weights"])
    gate = max(U.GATE_FACTOR * float(np.abs(s32["variances"] / s64["variances"] - 1.0).max()), 8.0 * 2.0 ** -23)
    err = float(np.abs(start["variances"] / s64["variances"] - 1.0).max())
    print(f"\nubm k {k} d {d} n {n} start: variances {err:.2e} / {gate:.2e}")
    assert err <= gate
    # "rows": EM from the restatement's float64 start (the library's own differs from it by rounding, which EM would carry into the gates)
    for tag, init in (("rows", s64), ("given", given)):
        want = U.fit(x, init, max_iter=8, tol=0.0, history=True)
        model = U.fit(x, init, max_iter=8, tol=0.0, dtype=np.float32, history=True)
        for iters in (1, 8):
            got = tr.fit(xd, init=init, max_iter=iters, tol=0.0)
            assert got["lower_bounds"].shape == (iters,)
            _check(got, _prefix(want, iters), _prefix(model, iters), f"k {k} d {d} n {n} {tag} iterations {iters}")
    if rows == "6000":                                                            # init=None is init_rows: the same bits as handing its output in
        _same(tr.fit(xd, max_iter=2, tol=0.0), tr.fit(xd, init=start, max_iter=2, tol=0.0), "init None")


@pytest.mark.parametrize("d", range(1, 17))
def test_every_d_of_the_dispatch(torch_cuda, d):
    """every d the statistics kernel is instantiated for, at k = 5 on one chunk and one row: one iteration at tol = 0 from a caller's
    start against float64, and twice the same bits"""
    import dsp_amd
    k, n = 5, U.CHUNK_ROWS + 1
    x, given = _case(k, d, n)
    xd = _cuda(torch_cuda, x)
    tr = dsp_amd.UbmTrainer(k, d)
    got = tr.fit(xd, init=given, max_iter=1, tol=0.0)
    want = U.fit(x, given, max_iter=1, tol=0.0, history=True)
    model = U.fit(x, given, max_iter=1, tol=0.0, dtype=np.float32, history=True)
    _check(got, _prefix(want, 1), _prefix(model, 1), f"k {k} d {d} n {n}")
    _same(tr.fit(xd, init=given, max_iter=1, tol=0.0), got, "every d twice")


@pytest.mark.parametrize("tag", ["iter1", "iter10", "tol"])
def test_fixture_against_sklearns_recorded_answers(torch_cuda, golden, tag):
    import dsp_amd
    z, x, init = fixture(golden)
    ref64, ref32 = fixture_fit(golden), fixture_fit(golden, np.float32)
    i, tol = int(z[f"{tag}__n_iter"]), float(z[f"{tag}__tol"])
    if tol > 0.0:       # the stop does not rest on a coin toss: no change of the lower bound up to it lies within 5 % of tol
        change = np.abs(np.diff(np.concatenate([[-np.inf], ref64["lower_bounds"]])))
        assert ref64["n_iter"] == ref32["n_iter"] == i and np.all(np.abs(change - tol) > 0.05 * tol)
    got = dsp_amd.UbmTrainer(32, 13).fit(_cuda(torch_cuda, x), init=init, max_iter=int(z[f"{tag}__max_iter"]), tol=tol, reg_covar=float(z["reg_covar"]))
    assert got["n_iter"] == i and got["converged"] == bool(z[f"{tag}__converged"])
    sk = U.result(z[f"{tag}__weights"], z[f"{tag}__means"], z[f"{tag}__variances"])
    sk.update(lower_bounds=np.array([float(z[f"{tag}__lower_bound"])]), n_iter=i, converged=bool(z[f"{tag}__converged"]))
    gates = U.gates(_prefix(ref32, i), _prefix(ref64, i))
    dev = U.deviations(dict(got, lower_bounds=got["lower_bounds"][-1:]), sk)
    print(f"\nubm fixture {tag}: " + ", ".join(f"{key} {dev[key]:.2e} / {gates[key]:.2e}" for key in gates) + "  (GPU vs sklearn / gate)")
    for key in gates:
        assert dev[key] <= gates[key], (tag, key, dev[key], gates[key])


def test_a_component_no_row_visits(torch_cuda):
    """one start mean at 1e3: it comes back with mean 0, variance reg_covar and a weight of about 1e-15 / n, as in sklearn; the others stay
    inside their gates"""
    import dsp_amd
    x, init = _case(5, 13, 2000)
    init["means"][2] = 1e3
    init["variances"][2] = 1.0
    want = U.fit(x, init, max_iter=3, tol=0.0, reg_covar=1e-5, history=True)
    model = U.fit(x, init, max_iter=3, tol=0.0, reg_covar=1e-5, dtype=np.float32, history=True)
    assert np.all(want["means"][2] == 0.0) and np.all(want["variances"][2] == 1e-5) and 0.0 < want["weights"][2] < 1e-17
    got = dsp_amd.UbmTrainer(5, 13).fit(_cuda(torch_cuda, x), init=init, max_iter=3, tol=0.0, reg_covar=1e-5)
    assert np.all(got["means"][2] == 0.0) and np.all(got["variances"][2] == 1e-5) and abs(got["weights"][2] / want["weights"][2] - 1.0) < 1e-6
    _check(got, _prefix(want, 3), _prefix(model, 3), "dead component")


def _fit_raw(torch, k, d, xd, init, max_iter, tol, reg_covar=1e-6, sentinel=777.0):
    """dsp_ubm_train_device itself, every result array pre-filled with `sentinel` -> (dict of the full arrays, n_iter, converged)"""
    import dsp_amd
    from dsp_amd import lib as dl
    tr = dsp_amd.UbmTrainer(k, d)
    keep = {key: np.ascontiguousarray(init[key], np.float64) for key in ("weights", "means", "variances")}
    out = {key: np.full(shape, sentinel) for key, shape in (("weights", k), ("means", (k, d)), ("variances", (k, d)), ("log_consts", k),
                                                            ("inv_covs", (k, d)), ("lower_bounds", max_iter))}
    res = dl.UbmResult()
    res.gmm.log_consts, res.gmm.means, res.gmm.inv_covs = (out[key].ctypes.data for key in ("log_consts", "means", "inv_covs"))
    res.weights, res.variances, res.lower_bounds = (out[key].ctypes.data for key in ("weights", "variances", "lower_bounds"))
    rc = tr._L.dsp_ubm_train_device(tr._h, xd.data_ptr(), xd.shape[0], C.byref(dl.UbmInit(*[keep[key].ctypes.data for key in ("weights", "means", "variances")])),
                                    C.byref(dl.UbmConfig(max_iter, tol, reg_covar)), C.byref(res), None)
    assert rc == 0, dl.last_error()
    assert res.gmm.k == k and res.gmm.d == d
    return out, int(res.n_iter), bool(res.converged)


def test_the_stop_is_honoured_by_the_launches_behind_it(torch_cuda, golden):
    """tol between two consecutive changes of the float64 lower bound on the fixture: n_iter and converged are the restatement's, the
    entries of lower_bounds past n_iter are untouched, and the model is the one after iteration n_iter -- not after max_iter"""
    z, x, init = fixture(golden)
    ref64, ref32 = fixture_fit(golden), fixture_fit(golden, np.float32)
    change = np.abs(np.diff(np.concatenate([[-np.inf], ref64["lower_bounds"]])))
    tol = float(np.sqrt(change[11] * change[12]))
    stop = int(np.flatnonzero(change < tol)[0])                                   # 0-based: n_iter = stop + 1
    change32 = np.abs(np.diff(np.concatenate([[-np.inf], ref32["lower_bounds"]])))
    assert 3 <= stop < 31 and np.all(np.abs(change[:stop + 1] - tol) > 0.05 * tol)
    assert int(np.flatnonzero(change32 < tol)[0]) == stop                         # (the float32 model agrees, as the 5 % margin promises)
    got, n_iter, converged = _fit_raw(torch_cuda, 32, 13, _cuda(torch_cuda, x), init, 40, tol)
    assert n_iter == stop + 1 and converged
    assert np.all(got["lower_bounds"][n_iter:] == 777.0) and np.all(got["lower_bounds"][:n_iter] != 777.0)
    full = dict(got, lower_bounds=got["lower_bounds"][:n_iter], n_iter=n_iter, converged=False)
    _check(full, _prefix(ref64, n_iter), _prefix(ref32, n_iter), f"stop after {n_iter} of 40")
    moved = float(np.abs(ref64["models"][n_iter + 7][1] - ref64["models"][n_iter - 1][1]).max())
    assert moved > 100 * U.gates(_prefix(ref32, n_iter), _prefix(ref64, n_iter))["means"]      # iterations behind the stop would have shown
    # max_iter reached without a stop: converged = 0, every entry written
    got, n_iter, converged = _fit_raw(torch_cuda, 32, 13, _cuda(torch_cuda, x), init, 5, 0.0)
    assert n_iter == 5 and not converged and np.all(got["lower_bounds"] != 777.0)


def test_bit_identity_across_calls_workspaces_addresses_and_trainers(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    k, d, n = 32, 13, 2 * GROUP_ROWS + 300
    x, given = _case(k, d, n)
    xd = _cuda(torch, x)
    tr = dsp_amd.UbmTrainer(k, d)
    for init in (None, given):
        kw = dict(init=init, max_iter=6, tol=0.0)
        first = tr.fit(xd, **kw)
        _same(tr.fit(xd, **kw), first, "the same call twice")
        tr.fit(_cuda(torch, np.concatenate([x[::-1]] * 3)), max_iter=2, tol=0.0)  # a larger problem grows the workspace and leaves its own sums there
        _same(tr.fit(xd, **kw), first, "after the workspace has grown")
        buf = torch.zeros(n * d + 8, dtype=torch.float32, device="cuda")
        moved = buf[1:1 + n * d].view(n, d)                                       # 4 bytes past a 16-byte boundary
        moved.copy_(xd)
        assert moved.data_ptr() % 16 == 4 and moved.is_contiguous()
        _same(tr.fit(moved, **kw), first, "rows at another address")
        _same(dsp_amd.UbmTrainer(k, d).fit(xd, **kw), first, "another trainer")
    start = tr.init_rows(xd)
    for key in start:
        assert np.array_equal(dsp_amd.UbmTrainer(k, d).init_rows(moved)[key], start[key]), key


def test_more_than_one_super_of_the_tree(torch_cuda):
    """32 groups and one row more: two supers, the second of one group of one row.  One iteration against float64, and twice the same bits"""
    import dsp_amd
    k, d, n = 5, 13, U.SUPER_GROUPS * GROUP_ROWS + 1
    x, given = _case(k, d, n)
    xd = _cuda(torch_cuda, x)
    tr = dsp_amd.UbmTrainer(k, d)
    got = tr.fit(xd, init=given, max_iter=1, tol=0.0)
    want = U.fit(x, given, max_iter=1, tol=0.0, history=True)
    model = U.fit(x, given, max_iter=1, tol=0.0, dtype=np.float32, history=True)
    _check(got, _prefix(want, 1), _prefix(model, 1), f"k {k} d {d} n {n}")
    _same(tr.fit(xd, init=given, max_iter=1, tol=0.0), got, "two supers twice")


def test_train_quantise_enrol_score(torch_cuda, golden):
    """the whole chain with nothing from outside the library: a population drawn from the reference UBM -> UbmTrainer.fit -> quantize_gmm ->
    SpeakerEnroller(fit result) -> two synthetic speakers enrolled -> SpeakerModel on the trained integer tables.  On held-out rows each
    speaker's own LLR mean exceeds the impostor's, and every LLR is exactly tests/consumer_ref.py's on the same tables"""
    import dsp_amd
    torch = torch_cuda
    z = golden("speaker_enroll_ref.npz")
    ref_ubm = {key: z[f"ubm_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
    rng = np.random.default_rng(7311)
    population = U.draw_population(rng, ref_ubm, 20000)
    ubm = dsp_amd.UbmTrainer(32, 13).fit(_cuda(torch, population), max_iter=30)
    assert ubm["n_iter"] >= 2 and np.all(np.diff(ubm["lower_bounds"]) > -1e-6) and abs(ubm["weights"].sum() - 1.0) < 1e-12
    assert np.isfinite(ubm["log_consts"]).all() and (ubm["variances"] >= 1e-6).all()
    ubm_int, saturated = dsp_amd.quantize_gmm(ubm)
    want_int, want_sat = U.quantize(ubm)
    assert all(np.array_equal(ubm_int[key], want_int[key]) for key in want_int) and saturated == want_sat
    assert saturated == {"means": 0, "inv_covs": 0, "log_consts": 0}
    spk = [E.draw_speaker(rng, ref_ubm, 1900) for _ in range(2)]
    train = np.concatenate([spk[0][:1500], spk[1][:1500]])
    held = np.concatenate([spk[0][1500:], spk[1][1500:]])
    out = dsp_amd.SpeakerEnroller(ubm).enroll(_cuda(torch, train), [0, 1500, 3000])
    q6 = out["means_q6"].cpu().numpy()
    assert int(out["saturated"].sum()) == 0
    for a in range(2):
        model = dsp_amd.SpeakerEnroller.speaker_model(q6[a], ubm_int)
        mean, label = model.llr_ragged(_cuda(torch, held), [0, 400, 800])
        mean = mean.cpu().numpy()
        target = {"means": q6[a], "inv_covs": ubm_int["inv_covs"], "log_consts": ubm_int["log_consts"]}
        want, want_label = R.speaker_means(target, ubm_int, held, [0, 400, 800])
        print(f"\ntrained UBM, speaker {a}: own {int(mean[a])}, impostor {int(mean[1 - a])} (Q8)")
        assert np.array_equal(mean, want) and np.array_equal(label.cpu().numpy(), want_label)
        assert mean[a] > mean[1 - a]
