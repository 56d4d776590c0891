"""GPU: sliding CMVN and MAP enrolment (dsp_cmvn_*, dsp_speaker_enroll*; dsp_amd.Cmvn, dsp_amd.SpeakerEnroller) against the float64
restatement of their definitions (tests/enroll_ref.py).

The gate, per output: a GPU value may deviate from float64 by GATE_FACTOR = 8 times what the restatement's own float32 model deviates on
the same inputs (computed here from tests/enroll_ref.py, never from the library; 8 covers another summation order and the hardware's
exp, log, sqrt and division at equal precision).  The Q6 means must equal the float64 Q6 value wherever that gate cannot move 64 * mean
across a rounding boundary (the tie zone, under 1 % of the entries).  Then what must hold bit for bit: a recording or speaker gives the
same outputs alone, in a batch, in the reversed batch and after the workspace has grown."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import consumer_ref as R
from tests import enroll_ref as E
from tests.enroll_util import MODES, build_main_enroll, fixture, write_wav

pytestmark = pytest.mark.gpu
KEYS = ("means", "means_q6", "counts", "ll_mean", "saturated")
LP = C.POINTER(C.c_long)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _offsets(lens, lead=0):
    return np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.int64)


def _cmvn_raw(torch, d, window, x, fo):
    """dsp_cmvn_ragged_device into a NaN-filled buffer with 2 spare rows behind the matrix -> numpy [rows + 2][d]"""
    import dsp_amd
    cm = dsp_amd.Cmvn(d, window)
    xin = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = torch.full((x.shape[0] + 2, d), float("nan"), dtype=torch.float32, device="cuda")
    rc = cm._L.dsp_cmvn_ragged_device(cm._h, xin.data_ptr(), len(fo) - 1, np.asarray(fo, np.int64).ctypes.data_as(LP), out.data_ptr(), None)
    assert rc == 0, dsp_amd.lib.last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


CMVN_CASES = {          # d, window, the recordings' lengths besides the silent one ("fixture": the golden's twelve in front)
    "fixture_d13_w300": (13, 300, "fixture"),
    "d1_w2": (1, 2, [0, 1, 2, 3, 63, 64, 65, 130]),
    "d16_w3": (16, 3, [1, 0, 2, 5, 64, 129]),
    "d13_w1024_long": (13, 1024, [3000, 1, 511, 513]),
    "d16_w300": (16, 300, [149, 150, 151, 365]),
    "d1_w300": (1, 300, [301, 64]),
    "d16_w2048_limit": (16, E.CMVN_MAX_WINDOW, [2200, 65]),      # the widest LDS image: 135 184 bytes
}


@pytest.mark.parametrize("case", list(CMVN_CASES))
def test_cmvn_parity_with_the_float64_definition(torch_cuda, golden, case):
    torch = torch_cuda
    d, window, lens = CMVN_CASES[case]
    rng = np.random.default_rng(len(case) + d * window)
    if lens == "fixture":
        z = fixture(golden)[0]
        recs = [z["raw_q"][a:b].astype(np.float32) / np.float32(32.0) for a, b in zip(z["frame_offsets"][:-1], z["frame_offsets"][1:])]
        recs += [np.zeros((0, d), np.float32)]
    else:       # rows shaped like compute_mfcc's: coefficient 0 in the hundreds, the others tens
        level = np.concatenate([[-450.0], rng.uniform(-40, 40, d - 1)])
        recs = [(level + rng.normal(0.0, 1.0, (n, d)) * np.concatenate([[90.0], rng.uniform(2, 30, d - 1)])).astype(np.float32) for n in lens]
    silent = len(recs)
    recs.append(np.zeros((40, d), np.float32))                                   # what compute_mfcc returns for silence
    recs.append(recs[2].copy() if lens == "fixture" else rng.normal(0, 5, (7, d)).astype(np.float32))
    lead = 3                                                                       # rows of no recording in front: every alignment
    x = np.concatenate([np.full((lead, d), 77.0, np.float32)] + recs)
    fo = _offsets([r.shape[0] for r in recs], lead)
    got = _cmvn_raw(torch, d, window, x, fo)
    assert np.isnan(got[:lead]).all() and np.isnan(got[fo[-1]:]).all(), "wrote outside the recordings"
    want = E.cmvn_ragged(x, fo, window)
    model = E.cmvn_ragged(x, fo, window, np.float32)
    gate = E.GATE_FACTOR * float(np.abs(model.astype(np.float64) - want).max())
    body = got[lead:fo[-1]].astype(np.float64)
    err = float(np.abs(body - want[lead:fo[-1]]).max())
    print(f"\ncmvn {case}: rows {int(fo[-1] - lead)}, gate {gate:.3e} (8 x the float32 model), GPU vs float64 {err:.3e}")
    assert np.isfinite(body).all() and gate > 0.0 and err <= gate
    assert np.all(got[fo[silent]:fo[silent + 1]] == 0.0)                          # silence: exact zeros
    for r, rec in enumerate(recs):
        if rec.shape[0] == 1:
            assert np.all(got[fo[r]:fo[r + 1]] == 0.0)                            # a one-row recording: exact zeros
    # a recording does not see its batch: alone, and in the reversed batch
    xr = np.concatenate(recs[::-1] + [np.zeros((1, d), np.float32)])
    fr = _offsets([r.shape[0] for r in recs[::-1]])
    rev = _cmvn_raw(torch, d, window, xr, fr)
    for r, rec in enumerate(recs):
        rr = len(recs) - 1 - r
        assert np.array_equal(rev[fr[rr]:fr[rr + 1]], got[fo[r]:fo[r + 1]]), (case, r)
        if rec.shape[0]:
            alone = _cmvn_raw(torch, d, window, rec, [0, rec.shape[0]])
            assert np.array_equal(alone[:rec.shape[0]], got[fo[r]:fo[r + 1]]), (case, r)


def _enroll(torch, en, feats, fo, kw):
    out = en.enroll(torch.from_numpy(np.ascontiguousarray(feats, np.float32)).cuda(), fo, **kw)
    torch.cuda.synchronize()
    return {key: out[key].cpu().numpy() for key in KEYS}


def _check_parity(got, feats, fo, ubm, kw, what):
    """the five outputs of a ragged enrolment against the float64 restatement under the 8 x rule; returns the gates"""
    want = E.enroll_ragged(feats, fo, ubm, **kw)
    model = E.enroll_ragged(feats, fo, ubm, dtype=np.float32, **kw)
    rows = np.diff(fo).astype(np.float64)
    dev = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())      # noqa: E731
    gates = {"means": E.GATE_FACTOR * dev(model["means"], want["means"]),
             "counts": E.GATE_FACTOR * dev(model["counts"] / rows[:, None], want["counts"] / rows[:, None]),
             "ll_mean": E.GATE_FACTOR * dev(model["ll_mean"], want["ll_mean"])}
    errs = {"means": dev(got["means"], want["means"]), "counts": dev(got["counts"] / rows[:, None], want["counts"] / rows[:, None]),
            "ll_mean": dev(got["ll_mean"], want["ll_mean"])}
    print(f"\nenroll {what}: gates " + ", ".join(f"{k} {v:.3e}" for k, v in gates.items()) + "; GPU vs float64 " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for key in gates:
        assert np.isfinite(got[key]).all() and errs[key] <= gates[key], (what, key, errs[key], gates[key])
    assert gates["means"] > 0.0 and gates["ll_mean"] > 0.0
    ties = E.tie_zone(want["means"], gates["means"])
    assert ties.mean() < 0.01, (what, float(ties.mean()))
    diff = np.abs(got["means_q6"].astype(int) - want["means_q6"].astype(int))
    assert np.all(diff[~ties] == 0) and np.all(diff <= 1), (what, int(diff.max()))
    q = np.rint(64.0 * want["means"])
    edge = (ties & ((q <= -128) | (q >= 127))).reshape(len(rows), -1).any(axis=1)          # a saturating entry in a tie zone
    assert np.array_equal(got["saturated"][~edge], want["saturated"][~edge]), what
    assert got["means_q6"].dtype == np.int8 and got["saturated"].dtype == np.int32
    return gates


@pytest.mark.parametrize("tag", list(MODES))
def test_enrolment_parity_on_the_fixture_speakers(torch_cuda, golden, tag):
    import dsp_amd
    z, ubm, feats = fixture(golden)
    got = _enroll(torch_cuda, dsp_amd.SpeakerEnroller(ubm), feats, z["frame_offsets"], MODES[tag])
    _check_parity(got, feats, z["frame_offsets"], ubm, MODES[tag], f"fixture {tag}")
    assert np.abs(got["means"] - z[f"{tag}__means"]).max() < 1e-3               # and the stored expectations are these


CHUNK_LENS = [E.CHUNK_ROWS - 1, E.CHUNK_ROWS, E.CHUNK_ROWS + 1, 2 * E.CHUNK_ROWS + 1]


SEED = 8        # under fixed alpha a component that hardly any row visits has an ill-conditioned mean F / N'; at this seed the float32 model's
                # deviation keeps the tie zone under 1 % for every (k, d) below (0.31 % at most: from tests/enroll_ref.py alone)


def _random_case(k, d):
    rng = np.random.default_rng(10000 * SEED + 100 * k + d)
    ubm = E.random_ubm(rng, k, d)
    feats = np.concatenate([E.draw_speaker(rng, ubm, n, 0.05) if k > 1 else E.draw_speaker(rng, ubm, n, 0.0, skip_floor=False) for n in CHUNK_LENS])
    return ubm, feats, _offsets(CHUNK_LENS)


@pytest.mark.parametrize("d", [1, 13, 16])
@pytest.mark.parametrize("k", [1, 5, 32, 64])
def test_chunk_edges_and_model_shapes(torch_cuda, k, d):
    """speakers of C - 1, C, C + 1 and 2 C + 1 rows (C = the kernel's rows per chunk) under random UBMs with variances log-uniform in
    [1e-6, 4] and one component at the floor; rows drawn from the UBM's wide components (k = 1: from its only one), moved by a speaker
    shift, as enrolment data lies where its UBM does"""
    import dsp_amd
    ubm, feats, fo = _random_case(k, d)
    assert np.isclose((1.0 / ubm["inv_covs"]).min(), 1e-6)
    en = dsp_amd.SpeakerEnroller(ubm)
    for tag, kw in MODES.items():
        _check_parity(_enroll(torch_cuda, en, feats, fo, kw), feats, fo, ubm, kw, f"k {k} d {d} {tag}")


@pytest.mark.parametrize("d", range(1, 17))
def test_every_d_of_the_dispatch(torch_cuda, d):
    """every d the statistics kernel is instantiated for, at k = 5: the chunk-edge speakers in both MAP modes.  (k = 5: the float32
    model's deviation keeps the tie zone at 0.36 % of the entries at most over these cases, from tests/enroll_ref.py alone; at k = 32 the
    ill-conditioned means of fixed alpha take it to 28 % at d = 10)"""
    import dsp_amd
    ubm, feats, fo = _random_case(5, d)
    en = dsp_amd.SpeakerEnroller(ubm)
    for tag, kw in MODES.items():
        _check_parity(_enroll(torch_cuda, en, feats, fo, kw), feats, fo, ubm, kw, f"k 5 d {d} {tag}")


DETERMINISM_CASES = ["fixture"] + [f"k{k}_d{d}" for k in (1, 5, 32, 64) for d in (1, 13, 16)]


@pytest.mark.parametrize("which", DETERMINISM_CASES)
def test_a_speaker_does_not_see_its_batch_or_the_workspace(torch_cuda, golden, which):
    """every speaker of the two parity tests above -- the fixture's twelve and the chunk-edge speakers of every (k, d) -- gives the same
    bits in all five outputs alone, in the batch, in the reversed batch and after a larger call has grown the workspace"""
    import dsp_amd
    torch = torch_cuda
    if which == "fixture":
        z, ubm, feats = fixture(golden)
        fo = z["frame_offsets"]
    else:
        ubm, feats, fo = _random_case(*(int(v) for v in re.fullmatch(r"k(\d+)_d(\d+)", which).groups()))
    n = len(fo) - 1
    parts = [feats[fo[s]:fo[s + 1]] for s in range(n)]
    for kw in MODES.values():
        en = dsp_amd.SpeakerEnroller(ubm)                                        # a fresh workspace: every call below grows it
        alone = [_enroll(torch, en, parts[s], [0, parts[s].shape[0]], kw) for s in range(n)]
        batch = _enroll(torch, en, feats, fo, kw)
        rev = _enroll(torch, en, np.concatenate(parts[::-1]), _offsets([p.shape[0] for p in parts[::-1]]), kw)
        _enroll(torch, en, np.concatenate([feats] * 3), _offsets(list(np.diff(fo)) * 3), kw)       # three times the chunks
        again = _enroll(torch, en, feats, fo, kw)
        for s in range(n):
            for key in KEYS:
                assert np.array_equal(alone[s][key][0], batch[key][s]), (which, s, key)
                assert np.array_equal(rev[key][n - 1 - s], batch[key][s]), (which, s, key)
                assert np.array_equal(again[key][s], batch[key][s]), (which, s, key)


def test_refusals_name_their_reason(torch_cuda, golden):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    L = dl.load()
    z, ubm, feats = fixture(golden)
    en = dsp_amd.SpeakerEnroller(ubm)
    x = torch.from_numpy(feats[:64].copy()).cuda()
    means = torch.zeros((3, 32, 13), device="cuda")
    off = lambda *a: (C.c_long * len(a))(*a)                                    # noqa: E731

    def call(n, offsets, cfg, out=means):
        return L.dsp_speaker_enroll_ragged_device(en._h, x.data_ptr(), n, offsets, C.byref(cfg), out.data_ptr() if out is not None else None,
                                                  None, None, None, None, None)

    def einval(rc, *words):
        assert rc == -1 and all(w in dl.last_error() for w in words), (rc, dl.last_error())

    ok = dl.EnrollConfig(dl.MAP_RELEVANCE, 16.0, 0.7)
    einval(call(3, off(0, 10, 10, 20), ok), "speaker 1", "no rows")
    einval(call(2, off(0, 10, 5), ok), "decrease")
    einval(call(1, off(-1, 10), ok), "non-negative")
    einval(call(1, off(0, 10), ok, out=None), "NULL")
    for r in (0.0, -1.0, float("nan"), float("inf")):
        einval(call(1, off(0, 10), dl.EnrollConfig(dl.MAP_RELEVANCE, r, 0.7)), "relevance_factor")
    for a in (-0.01, 1.01, float("nan")):
        einval(call(1, off(0, 10), dl.EnrollConfig(dl.MAP_FIXED_ALPHA, 16.0, a)), "fixed_alpha")
    einval(call(1, off(0, 10), dl.EnrollConfig(7, 16.0, 0.7)), "map_mode")
    assert call(1, off(0, 10), dl.EnrollConfig(dl.MAP_FIXED_ALPHA, -5.0, 1.0)) == 0      # each mode reads its own parameter
    assert call(0, None, ok) == 0 and call(0, None, ok, out=None) == 0                  # zero speakers: DSP_OK, no launch
    h = C.c_void_p()
    arr = np.ones(65 * 17)
    for k, d, word in ((65, 13, "64"), (32, 17, "16")):
        rc = L.dsp_speaker_enroller_create(C.byref(dl.GmmFloatParams(k, d, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)), 0, C.byref(h))
        einval(rc, word)
    einval(L.dsp_cmvn_create(0, 13, 1, C.byref(h)), "window")
    einval(L.dsp_cmvn_create(0, 13, E.CMVN_MAX_WINDOW + 1, C.byref(h)), str(E.CMVN_MAX_WINDOW))
    cm = dsp_amd.Cmvn(13, 300)
    y = torch.full_like(x, 5.0)
    einval(L.dsp_cmvn_ragged_device(cm._h, x.data_ptr(), 1, off(0, 64), x.data_ptr(), None), "alias")          # in place
    einval(L.dsp_cmvn_ragged_device(cm._h, x.data_ptr(), 2, off(0, 40, 30), y.data_ptr(), None), "decrease")
    assert L.dsp_cmvn_ragged_device(cm._h, None, 0, None, None, None) == 0
    assert L.dsp_cmvn_ragged_device(cm._h, x.data_ptr(), 3, off(5, 5, 5, 5), y.data_ptr(), None) == 0          # recordings without rows
    torch.cuda.synchronize()
    assert bool((y == 5.0).all()) and bool((means[1:] == 0.0).all())            # no refused or empty call wrote anything
    assert bool(torch.isfinite(means[0]).all()) and bool((means[0] != 0.0).any())           # (the one accepted call enrolled speaker 0)
    with pytest.raises(ValueError):
        en.enroll(x, [0, 10, 10, 20])
    assert dsp_amd.Cmvn(13, 1024).window == 1024


def test_enrolled_tables_through_the_integer_scorer(torch_cuda, golden):
    """two synthetic speakers drawn from the reference UBM (tests/enroll_ref.py draw_speaker, seed fixed here; the float64 restatement's
    gap on this seed: 470 .. 540 Q8 units), 1 500 rows each enrolled on the GPU, a SpeakerModel from each speaker's means_q6 and the
    golden UBM's int tables: on 400 held-out rows the speaker's own LLR mean exceeds the impostor's, and every LLR mean is exactly
    tests/consumer_ref.py's on the GPU-enrolled tables -- the tables are consumable and the scorer is what it was"""
    import dsp_amd
    torch = torch_cuda
    z, ubm, _ = fixture(golden)
    s = golden("speaker_gmm_ref.npz")
    ubm_int = {key: s[f"ubm_{key}"] for key in ("means", "inv_covs", "log_consts")}
    rng = np.random.default_rng(4102)
    spk = [E.draw_speaker(rng, ubm, 1900) for _ in range(2)]
    train = np.concatenate([spk[0][:1500], spk[1][:1500]])
    held = np.concatenate([spk[0][1500:], spk[1][1500:]])
    en = dsp_amd.SpeakerEnroller(ubm)
    for tag, kw in MODES.items():
        out = _enroll(torch, en, train, [0, 1500, 3000], kw)
        for a in range(2):
            model = dsp_amd.SpeakerEnroller.speaker_model(out["means_q6"][a], ubm_int)
            mean, label = model.llr_ragged(torch.from_numpy(held).cuda(), [0, 400, 800])
            mean = mean.cpu().numpy()
            target = {"means": out["means_q6"][a], "inv_covs": ubm_int["inv_covs"], "log_consts": ubm_int["log_consts"]}
            want, want_label = R.speaker_means(target, ubm_int, held, [0, 400, 800])
            print(f"\n{tag} speaker {a}: own {int(mean[a])}, impostor {int(mean[1 - a])} (Q8)")
            assert np.array_equal(mean, want) and np.array_equal(label.cpu().numpy(), want_label)
            assert mean[a] > mean[1 - a]


def test_full_chain_from_samples(torch_cuda, golden):
    """two short ragged recordings -> dsp_mfcc_clips_ragged_device -> Cmvn -> enroll"""
    import dsp_amd
    torch = torch_cuda
    _, ubm, _ = fixture(golden)
    rng = np.random.default_rng(5)
    lens = [16000 * 2 + 123, 16000 + 7]
    env = np.repeat(rng.uniform(0.05, 1.0, sum(lens) // 400 + 1), 400)[:sum(lens)]
    signal = torch.from_numpy((rng.uniform(-1, 1, sum(lens)) * env).astype(np.float32)).cuda()
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    mfcc, fo = plan.clips_ragged(signal, _offsets(lens), 2**31 - 1)
    assert mfcc.shape[1] == 13 and np.diff(fo).min() >= 98
    feats = dsp_amd.Cmvn(13).apply(mfcc, fo)
    want = E.cmvn_ragged(mfcc.cpu().numpy(), fo, 300)
    model = E.cmvn_ragged(mfcc.cpu().numpy(), fo, 300, np.float32)
    gate = E.GATE_FACTOR * float(np.abs(model - want).max())
    assert float(np.abs(feats.cpu().numpy() - want).max()) <= gate
    out = dsp_amd.SpeakerEnroller(ubm).enroll(feats, fo)
    x = feats.cpu().numpy()
    w64 = E.enroll_ragged(x, fo, ubm)
    m32 = E.enroll_ragged(x, fo, ubm, dtype=np.float32)
    rows = np.diff(fo).astype(np.float64)
    count_gate = E.GATE_FACTOR * float(np.abs(m32["counts"] / rows[:, None] - w64["counts"] / rows[:, None]).max())
    counts = out["counts"].cpu().numpy().astype(np.float64)
    assert bool(torch.isfinite(out["means"]).all()) and out["means"].shape == (2, 32, 13)
    err = float(np.abs(counts.sum(axis=1) / rows - 1.0).max())
    print(f"\nfull chain: rows {rows.tolist()}, counts gate {count_gate:.3e}, | sum_k counts / rows - 1 | {err:.3e}")
    assert count_gate > 0.0 and err <= count_gate


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_example_main_enroll_prints_the_python_chains_tables(torch_cuda, golden, tmp_path):
    """examples/main_enroll.c on two WAV files of one speaker against the same chain through the Python wrappers: the same entry points
    on the same bytes, so the printed Q6 means are the wrappers' means_q6 exactly; the other two tables are the float UBM's, rounded"""
    import dsp_amd
    torch = torch_cuda
    _, ubm, _ = fixture(golden)
    exe = build_main_enroll(str(tmp_path / "main_enroll"))
    (tmp_path / "ubm.txt").write_text("32 13\n" + "\n".join(repr(float(v)) for key in ("log_consts", "means", "inv_covs") for v in ubm[key].reshape(-1)) + "\n")
    rng = np.random.default_rng(9)
    lens = [16000 * 2 + 77, 16000 + 5]
    pcm = [np.rint(rng.uniform(-1, 1, n) * np.repeat(rng.uniform(500, 20000, n // 400 + 1), 400)[:n]).astype(np.int16) for n in lens]
    for i, x in enumerate(pcm):
        write_wav(str(tmp_path / f"f{i}.wav"), x)
    r = subprocess.run([exe, str(tmp_path / "ubm.txt"), str(tmp_path / "f0.wav"), str(tmp_path / "f1.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def table(name):
        body = re.search(name + r"(?:\[\w+\])+ = \{(.*?)\};", r.stdout, re.S).group(1)
        return np.array([int(v) for v in re.findall(r"-?\d+", body)])

    x16, oo = dsp_amd.Resampler(16000, 16000).ragged(torch.from_numpy(np.concatenate(pcm)).cuda(), _offsets(lens))
    mfcc, fo = dsp_amd.MfccPlan(dsp_amd.default_config()).clips_ragged(x16, oo, 2**31 - 1)
    out = dsp_amd.SpeakerEnroller(ubm).enroll(dsp_amd.Cmvn(13).apply(mfcc, fo), [fo[0], fo[-1]])
    assert np.array_equal(table("target_means"), out["means_q6"].cpu().numpy().reshape(-1).astype(int))
    assert np.array_equal(table("target_log_consts"), np.rint(ubm["log_consts"] * 256).astype(int))
    assert np.array_equal(table("target_inv_covs"), np.rint(ubm["inv_covs"] * 2048).astype(int).reshape(-1))
    assert f"{int(fo[-1])} rows" in r.stdout
