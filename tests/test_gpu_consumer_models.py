"""GPU: the stop net and the speaker GMM on seeded random models, through every entry path, against the plain numpy references
of tests/consumer_ref.py (pinned to the oracle by tests/test_consumer_ref_cpu.py).

Stop models span n_coef 1 / 13 / 20, max_frames 1 / 7 / 16 / 17 / 98 / 500 / 1260 / 1261 and first layers of 1 / 2 / 3 / 4 / 5 / 16
units (STOP_MODELS, seed 1000 + index); each path's P("stop") must lie within 1e-6 of the reference, which differs from the kernels
only in the order of their float64 layer-1 sums (and, on the fused path, in the scaler folded into the weights).  The scan's
(window, hop) pairs run every tile width for the golden model and a 16-unit one:

    (98, 10) -> 64   (1, 1) -> 64   (98, 40) -> 16   (600, 30) -> 16   (98, 100) -> 4   (98, 400) -> 1   (600, 300) -> 1

The fused and ragged fused paths run on every model with units[0] <= 4 and n_coef <= 16 -- the n_coef 13 ones and, beyond the
reference's shape, the n_coef 1 ones, since the library accepts plans of up to 16 coefficients there; the others must be refused.
The fused epilogue's other float instantiations (gather 6; gather 3 at a run-time frame length) run in
test_fused_ragged_on_other_instantiations.

GMMs span K 1 / 2 / 31 / 64 and D 1 / 7 / 13 / 16 (seed 100 K + D); every speaker result must equal the reference exactly."""
import numpy as np
import pytest

from tests import consumer_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
PTOL = 1e-6
NO_CAP = 2**31 - 1
HOP, FRAME = 160, 400

# (n_coef, max_frames, units): every value of each range at least once
STOP_MODELS = [(13, 500, (4, 2, 2, 1)), (13, 98, (1, 1, 1, 1)), (13, 17, (2, 3, 2, 1)), (13, 16, (3, 16, 4, 1)), (13, 7, (4, 4, 16, 1)),
               (13, 1, (2, 2, 2, 1)), (13, 1260, (3, 5, 2, 1)), (13, 1261, (1, 2, 1, 1)), (13, 500, (16, 16, 16, 1)), (13, 98, (5, 3, 2, 1)),
               (1, 1, (1, 1, 1, 1)), (1, 500, (16, 8, 3, 1)), (1, 1261, (4, 2, 2, 1)), (20, 17, (5, 4, 4, 1)), (20, 1260, (2, 16, 1, 1)),
               (20, 7, (16, 1, 16, 1)), (20, 98, (3, 2, 2, 1)), (1, 16, (3, 3, 3, 1))]
# the fused epilogue takes first layers of <= 4 units on plans of the reference's MFCC shape: 40 mels, n_mfcc <= 16 (n_mfcc 20 splits
# its DCT differently and is refused)
FUSED = [i for i, (nc, _mf, u) in enumerate(STOP_MODELS) if nc <= 16 and u[0] <= 4]
SIXTEEN = 8
TILES = [(98, 10, 64), (1, 1, 64), (98, 40, 16), (600, 30, 16), (98, 100, 4), (98, 400, 1), (600, 300, 1)]
GMM_SHAPES = [(k, d) for k in (1, 2, 31, 64) for d in (1, 7, 13, 16)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _check_p(got, want, bound, what):
    """|dP| <= 1e-6; a miss names the first-order bound of a 2^-22 relative error per layer-1 term, to tell rounding from a bug"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    if not (err <= PTOL).all():
        k = int(np.nanargmax(np.where(np.isnan(err), np.inf, err)))
        raise AssertionError(f"{what}: |dP| = {err[k]:.3e} at {k} (kernel {got[k]!r}, reference {want[k]!r}); first-order rounding bound "
                             f"2^-22 sum|w xs| prod||W_l||inf / 4 = {bound[k]:.3e}; {int((~(err <= PTOL)).sum())} of {err.size} miss")


def _not_vacuous(probs):
    p = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in probs])
    assert np.mean((p >= 0.01) & (p <= 0.99)) >= 1 / 3, f"draw on a plateau: {np.mean((p >= 0.01) & (p <= 0.99)):.2f} of P in [0.01, 0.99]"


def _draw(i, loc=None, spread=None):
    """model i of STOP_MODELS (seed 1000 + i) for data of the given shape, or of a seeded one -> (rng, model, (loc, spread))"""
    rng = np.random.default_rng(1000 + i)
    nc, mf, units = STOP_MODELS[i]
    if loc is None:
        loc, spread = R.stop_data_shape(rng, nc)
    return rng, R.random_stop_model(rng, nc, mf, units, loc, spread), (loc, spread)


def _golden_rows(m, rng, n):
    """rows like the golden scaler's data: coefficient c about its mean scaler mean, +- its mean scale"""
    mean = np.asarray(m["scaler_mean"], np.float64).reshape(13, 500).mean(axis=1)
    scale = np.asarray(m["scaler_scale"], np.float64).reshape(13, 500).mean(axis=1)
    return (mean + scale * rng.standard_normal((n, 13))).astype(F32)


def _ragged(rng, lens, shape, lead, fill):
    """a ragged matrix of rows of the data shape whose recordings of `lens` rows start at row `lead`; the rows before and after
    them hold `fill`"""
    fo = lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mf = np.full((int(fo[-1]) + 5, shape[0].size), fill, F32)
    mf[lead:fo[-1]] = R.stop_rows(rng, shape, int(fo[-1]) - lead)
    return mf, fo


# ---- stop net ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(STOP_MODELS)))
def test_predict_random_models(torch_cuda, i):
    """dsp_stop_predict_device (stop_tail_kernel) on T = 0, 1, max_frames - 1 .. max_frames + 9"""
    import dsp_amd
    torch = torch_cuda
    rng, m, shape = _draw(i)
    _nc, mf, _u = STOP_MODELS[i]
    ts = sorted({0, 1, max(1, mf - 1), mf, mf + 1, mf + 9})
    mats = {t: np.stack([R.stop_rows(rng, shape, t) for _ in range(4)]) for t in ts}
    m = R.fit_biases(rng, m, [x for t in ts for x in mats[t]])
    net, ref = dsp_amd.StopModel(m), R.StopNet(m)
    probs = []
    for t in ts:
        got = net.predict(torch.from_numpy(mats[t]).cuda()).cpu().numpy()
        want = [ref.prob(x) for x in mats[t]]
        _check_p(got, [p for p, _b in want], [b for _p, b in want], f"model {i} {STOP_MODELS[i]} predict T={t}")
        probs.append(got)
    _not_vacuous(probs)


@pytest.mark.parametrize("wf,hop,tw", TILES)
def test_scan_every_tile_width(torch_cuda, golden, wf, hop, tw):
    """StopModel.scan at each tile width, golden model and a 16-unit one: recordings of 0, window - 1, window, window + hop - 1
    rows and two of more than two tiles; the matrix starts 37 NaN rows in (frame_offsets[0] > 0) and ends in NaN rows"""
    import dsp_amd
    torch = torch_cuda
    probs = []
    for name in ("golden", "sixteen"):
        if name == "golden":
            rng, m = np.random.default_rng(wf * 1000 + hop), dict(golden("stop_model.npz"))
            shape = (np.zeros(13), np.ones(13))
        else:
            rng, m, shape = _draw(SIXTEEN)
        assert R.stop_scan_tile(13, 500, int(np.asarray(m["bias0"]).size), wf, hop) == tw
        lens = [0, wf - 1, wf, wf + hop - 1, wf + hop * (2 * tw + 5) + 3, wf + hop * tw + 1]
        mfm, fo = _ragged(rng, lens, shape, 37, np.nan)
        if name == "golden":
            mfm[37:fo[-1]] = _golden_rows(m, rng, int(fo[-1]) - 37)
        else:
            m = R.fit_biases(rng, m, [mfm[s:s + n] for (_r, s, n) in R.scan_windows(fo, wf, hop)])
        net, ref = dsp_amd.StopModel(m), R.StopNet(m)
        wo, prob = net.scan(torch.from_numpy(mfm).cuda(), fo, wf, hop)
        assert np.diff(wo).tolist() == [1 if n < wf else 1 + (n - wf) // hop for n in lens]
        want, bound = R.stop_scan(ref, mfm, fo, wf, hop)
        _check_p(prob.cpu().numpy(), want, bound, f"{name} scan ({wf}, {hop}) TW {tw}")
        probs.append(prob.cpu().numpy())
    _not_vacuous(probs)


@pytest.mark.parametrize("i", range(len(STOP_MODELS)))
def test_scan_random_models(torch_cuda, i):
    """StopModel.scan on each random model: a seeded window of 1-130 rows (longer than some models' max_frames), a hop up to
    past the window, the edge recordings, a start past row 0"""
    import dsp_amd
    torch = torch_cuda
    rng, m, shape = _draw(i)
    nc, mf_, u = STOP_MODELS[i]
    wf = int(rng.integers(1, 131))
    hop = int(rng.integers(1, 2 * wf + 4))
    tw = R.stop_scan_tile(nc, mf_, u[0], wf, hop)
    assert tw > 0
    lens = [0, wf - 1, wf, wf + hop - 1, int(rng.integers(wf, wf + 70 * hop))]
    mfm, fo = _ragged(rng, lens, shape, int(rng.integers(1, 50)), np.nan)
    m = R.fit_biases(rng, m, [mfm[s:s + n] for (_r, s, n) in R.scan_windows(fo, wf, hop)])
    net, ref = dsp_amd.StopModel(m), R.StopNet(m)
    _wo, prob = net.scan(torch.from_numpy(mfm).cuda(), fo, wf, hop)
    want, bound = R.stop_scan(ref, mfm, fo, wf, hop)
    prob = prob.cpu().numpy()
    _check_p(prob, want, bound, f"model {i} {STOP_MODELS[i]} scan ({wf}, {hop}) TW {tw}")
    _not_vacuous([prob])


def test_scan_lds_limit(torch_cuda):
    """max_frames 1260 x 13 coefficients fill the scan block's 64 KiB (TW 1); 1261 rows do not fit: scan and Scanner refuse by name"""
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    i_fit, i_over = STOP_MODELS.index((13, 1260, (3, 5, 2, 1))), STOP_MODELS.index((13, 1261, (1, 2, 1, 1)))
    rng, m, shape = _draw(i_fit)
    wf, hop = 1300, 2
    assert R.stop_scan_tile(13, 1260, 3, wf, hop) == 1 and 1260 * 13 * 4 <= 65536 < 1261 * 13 * 4
    mfm, fo = _ragged(rng, [wf + 9, 1260, 1259], shape, 3, np.nan)
    m = R.fit_biases(rng, m, [mfm[s:s + n] for (_r, s, n) in R.scan_windows(fo, wf, hop)])
    net, ref = dsp_amd.StopModel(m), R.StopNet(m)
    _wo, prob = net.scan(torch.from_numpy(mfm).cuda(), fo, wf, hop)
    want, bound = R.stop_scan(ref, mfm, fo, wf, hop)
    _check_p(prob.cpu().numpy(), want, bound, "max_frames 1260 scan")
    _not_vacuous([prob.cpu().numpy()])
    _rng, m, _shape = _draw(i_over, *shape)
    m = R.fit_biases(rng, m, [mfm[s:s + n] for (_r, s, n) in R.scan_windows(fo, 1260, 1)])
    over = dsp_amd.StopModel(m)
    with pytest.raises(L.DspError, match="does not fit the scan kernel's LDS"):
        over.scan(torch.from_numpy(mfm).cuda(), fo, 1261, 1)
    with pytest.raises(L.DspError, match="does not fit the scan kernel's LDS"):
        dsp_amd.Scanner(plan, stop=over, window_frames=1261, hop_frames=1)
    _wo, prob = over.scan(torch.from_numpy(mfm).cuda(), fo, 1260, 1)          # a window of 1260 rows still fits
    want, bound = R.stop_scan(R.StopNet(m), mfm, fo, 1260, 1)
    _check_p(prob.cpu().numpy(), want, bound, "max_frames 1261 model, window 1260")
    _not_vacuous([prob.cpu().numpy()])


def _noise_clips(rng, lens):
    out = []
    for n in lens:
        x = rng.uniform(-1, 1, n).astype(F32)
        env = np.repeat(rng.uniform(0.01, 1.0, n // 1600 + 1).astype(F32), 1600)[:n]
        out.append((x * env).astype(F32))
    return out


def _clip_mfcc(torch, plan, clip, max_frames):
    """the MFCC the net sees: the clip path's matrix, capped at max_frames (the ragged and fused paths are bit-exact to it)"""
    if clip.size < FRAME:
        return np.zeros((0, plan.cfg.n_mfcc), F32)
    return plan.clips(torch.from_numpy(clip).cuda()[None], max_frames)[0].cpu().numpy()


@pytest.mark.parametrize("i", FUSED)
def test_fused_paths_random_models(torch_cuda, monkeypatch, i):
    """classify_signal_batch on the fused epilogue and on the two-kernel path, and classify_signal_ragged, on PCM clips of
    max_frames - 1 .. max_frames + 3 frames (and, ragged, a clip of 1 frame; one of none is refused); the reference runs on
    plan.clips' MFCC"""
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    nc, mf, units = STOP_MODELS[i]
    plan = dsp_amd.MfccPlan(dsp_amd.default_config(n_mfcc=nc))
    rng = np.random.default_rng(2000 + i)
    ts = sorted({max(1, mf - 1), mf, mf + 3})
    # even lengths: the uniform entry runs fused only on an even clip stride
    groups = {t: _noise_clips(rng, [FRAME + (t - 1) * HOP + 2 * int(rng.integers(0, HOP // 2))] * 3) for t in ts}
    extra = _noise_clips(rng, [FRAME - 1, FRAME, FRAME + (mf + 1) * HOP + 17])
    mats = {t: [_clip_mfcc(torch, plan, c, mf) for c in cs] for t, cs in groups.items()}
    extra_mats = [_clip_mfcc(torch, plan, c, mf) for c in extra]
    allm = np.concatenate([x for t in ts for x in mats[t]])
    _rng, m, _shape = _draw(i, allm.mean(axis=0), allm.std(axis=0) + 1e-3)
    m = R.fit_biases(rng, m, [x for t in ts for x in mats[t]] + extra_mats)
    net, ref = dsp_amd.StopModel(m), R.StopNet(m)
    probs = []
    for t in ts:
        batch = torch.from_numpy(np.stack(groups[t])).cuda()
        want = [ref.prob(x) for x in mats[t]]
        wp, wb = [p for p, _b in want], [b for _p, b in want]
        # The uniform entry does not say which path ran: it falls back to the two kernels without a word on an odd clip stride, a
        # misaligned buffer or a plan outside the fused shape (stop_fused_device).  So the test holds the fused preconditions itself,
        # and runs the same clips through the ragged entry, which refuses instead of falling back: that call proves the fused
        # epilogue ran on them.
        assert batch.stride(0) % 2 == 0 and batch.data_ptr() % 8 == 0 and units[0] <= 4
        fused = net.classify_signal_batch(plan, batch).cpu().numpy()
        _check_p(fused, wp, wb, f"model {i} {STOP_MODELS[i]} uniform entry (fused preconditions held) T={t}")
        n_s = groups[t][0].size
        same = net.classify_signal_ragged(plan, batch.reshape(-1), np.arange(len(groups[t]) + 1, dtype=np.int64) * n_s).cpu().numpy()
        _check_p(same, wp, wb, f"model {i} {STOP_MODELS[i]} ragged fused, equal clips T={t}")
        monkeypatch.setenv("DSP_AMD_STOP_TWO_KERNELS", "1")
        two = net.classify_signal_batch(plan, batch).cpu().numpy()
        monkeypatch.delenv("DSP_AMD_STOP_TWO_KERNELS")
        _check_p(two, wp, wb, f"model {i} {STOP_MODELS[i]} two-kernel T={t}")
        probs += [fused, same, two]
    clips = [c for t in ts for c in groups[t]] + extra
    order = rng.permutation(len(clips))
    clips, cmats = [clips[k] for k in order], [([x for t in ts for x in mats[t]] + extra_mats)[k] for k in order]
    offsets = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    short = [k for k, c in enumerate(clips) if c.size < FRAME]
    with pytest.raises(L.DspError, match=f"clip {short[0]} of the ragged batch is shorter than one frame"):      # every clip needs a frame
        net.classify_signal_ragged(plan, torch.from_numpy(np.concatenate(clips)).cuda(), offsets)
    clips, cmats = [c for k, c in enumerate(clips) if k not in short], [x for k, x in enumerate(cmats) if k not in short]
    offsets = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    rag = net.classify_signal_ragged(plan, torch.from_numpy(np.concatenate(clips)).cuda(), offsets).cpu().numpy()
    want = [ref.prob(x) for x in cmats]
    _check_p(rag, [p for p, _b in want], [b for _p, b in want], f"model {i} {STOP_MODELS[i]} ragged fused")
    probs.append(rag)
    _not_vacuous(probs)


@pytest.mark.parametrize("i", [i for i in range(len(STOP_MODELS)) if i not in FUSED])
def test_outside_the_fused_shape(torch_cuda, i):
    """units[0] > 4 or n_coef 20: the ragged entry refuses with its reason; the uniform entry runs the two-kernel path"""
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    nc, mf, _u = STOP_MODELS[i]
    plan = dsp_amd.MfccPlan(dsp_amd.default_config(n_mfcc=nc))
    rng = np.random.default_rng(3000 + i)
    t = min(mf, 40)
    clips = _noise_clips(rng, [FRAME + (t - 1) * HOP] * 4)
    mats = [plan.clips(torch.from_numpy(c).cuda()[None], mf)[0].cpu().numpy() for c in clips]
    allm = np.concatenate(mats)
    _rng, m, _shape = _draw(i, allm.mean(axis=0), allm.std(axis=0) + 1e-3)
    m = R.fit_biases(rng, m, mats)
    net, ref = dsp_amd.StopModel(m), R.StopNet(m)
    sig = torch.from_numpy(np.concatenate(clips)).cuda()
    with pytest.raises(L.DspError, match="ragged batches run on the fused clip"):
        net.classify_signal_ragged(plan, sig, [0, clips[0].size, 2 * clips[0].size])
    got = net.classify_signal_batch(plan, torch.from_numpy(np.stack(clips)).cuda()).cpu().numpy()
    want = [ref.prob(x) for x in mats]
    _check_p(got, [p for p, _b in want], [b for _p, b in want], f"model {i} {STOP_MODELS[i]} uniform batch")


# the fused epilogue's other two float instantiations (fused_form_one, mfcc_kernels.hip): gather 6 and gather 3 with the run-time
# frame length -- name -> (default_config overrides, (dct_split, dct_len, mel_gather) the plan must select)
FUSED_OTHER_SHAPES = {"mels32": (dict(n_mels=32), (4, 10, 6)), "flen320": (dict(frame_length=320), (4, 10, 3))}


@pytest.mark.parametrize("which", list(FUSED_OTHER_SHAPES))
def test_fused_ragged_on_other_instantiations(torch_cuda, which):
    """classify_signal_ragged -- it refuses rather than falling back, so the fused epilogue ran -- with a 13-coefficient model on a
    32-filter bank (<4,10,6,0,...,2>) and on the default bank at frame length 320 (<4,10,3,0,...,2>): clips of max_frames - 1 ..
    max_frames + 3 frames and one of a single frame, in seeded order; the reference runs on plan.clips' MFCC"""
    import ctypes as C
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    over, shape = FUSED_OTHER_SHAPES[which]
    nc, mf, units = 13, 17, (4, 3, 2, 1)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config(**over))
    t = L.LaneTables512()
    assert plan._L.dsp_mfcc_lane_tables(C.byref(plan.cfg), C.byref(t), C.sizeof(t)) == 0
    assert (t.dct_split, t.dct_len, t.mel_gather) == shape
    frame = plan.cfg.frame_length
    rng = np.random.default_rng(2100 + len(which))
    lens = [frame + (k - 1) * HOP + int(rng.integers(0, HOP)) for k in (mf - 1, mf, mf, mf + 3, 1, mf + 1)]
    clips = _noise_clips(rng, lens)
    mats = [plan.clips(torch.from_numpy(c).cuda()[None], mf)[0].cpu().numpy() for c in clips]
    assert [x.shape[0] for x in mats] == [mf - 1, mf, mf, mf, 1, mf]
    allm = np.concatenate(mats)
    m = R.random_stop_model(rng, nc, mf, units, allm.mean(axis=0), allm.std(axis=0) + 1e-3)
    m = R.fit_biases(rng, m, mats)
    net, ref = dsp_amd.StopModel(m), R.StopNet(m)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    got = net.classify_signal_ragged(plan, torch.from_numpy(np.concatenate(clips)).cuda(), offsets).cpu().numpy()
    want = [ref.prob(x) for x in mats]
    _check_p(got, [p for p, _b in want], [b for _p, b in want], f"fused ragged on {which} {shape}")
    _not_vacuous([got])


# ---- speaker GMM ------------------------------------------------------------------------------------------------------------

def _speaker(k, d, salt=0):
    import dsp_amd
    rng = np.random.default_rng(100 * k + d + salt)
    t, u = R.random_gmm(rng, k, d), R.random_gmm(rng, k, d)
    return rng, t, u, dsp_amd.SpeakerModel(t, u)


@pytest.mark.parametrize("k,d", GMM_SHAPES)
def test_speaker_every_path_random_gmms(torch_cuda, k, d):
    """llr and llr_ragged (per-frame outputs included) and SpeakerModel.scan, every window, on inputs with Q6 edge values"""
    torch = torch_cuda
    rng, t, u, spk = _speaker(k, d)
    x = R.speaker_inputs(rng, 5 * 77, d).reshape(5, 77, d)
    x[0, 0] = R.Q6_EDGES[np.arange(d) % R.Q6_EDGES.size]
    mean, label, lt, lu = spk.llr(torch.from_numpy(x).cuda(), per_frame=True)
    rlt, rlu = R.speaker_rows(t, u, x.reshape(-1, d))
    assert np.array_equal(lt.cpu().numpy().reshape(-1), rlt) and np.array_equal(lu.cpu().numpy().reshape(-1), rlu)
    rm, rl = R.speaker_means(t, u, x.reshape(-1, d), np.arange(6) * 77)
    assert np.array_equal(mean.cpu().numpy(), rm) and np.array_equal(label.cpu().numpy(), rl)
    # ragged: clips of 1, 63, 64, 65, 200 and 7 rows from row 11 of a matrix whose other rows would wrap in Q6
    lens = [1, 63, 64, 65, 200, 7]
    fo = 11 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mf = np.full((int(fo[-1]) + 3, d), 1000.0, F32)
    mf[11:fo[-1]] = R.speaker_inputs(rng, int(fo[-1]) - 11, d)
    mean, label, lt, lu = spk.llr_ragged(torch.from_numpy(mf).cuda(), fo, per_frame=True)
    rlt, rlu = R.speaker_rows(t, u, mf[11:fo[-1]])
    assert np.array_equal(lt.cpu().numpy()[11:], rlt) and np.array_equal(lu.cpu().numpy()[11:], rlu)
    rm, rl = R.speaker_means(t, u, mf, fo)
    assert np.array_equal(mean.cpu().numpy(), rm) and np.array_equal(label.cpu().numpy(), rl)
    # scan: window 98, hop 10 and hop 150 (> window) over the same recordings
    for wf, hop in ((98, 10), (98, 150), (1, 1)):
        wo, sm, sl = spk.scan(torch.from_numpy(mf).cuda(), fo, wf, hop)
        rm, rl = R.speaker_scan(t, u, mf, fo, wf, hop)
        assert int(wo[-1]) == rm.size
        assert np.array_equal(sm.cpu().numpy(), rm) and np.array_equal(sl.cpu().numpy(), rl), (wf, hop)
    assert len(set(rl.tolist())) == 2 or k == 1, "labels all alike"


def test_speaker_scan_past_256_chunks(torch_cuda):
    """> 262 144 rows (more than 256 chunks of 1024: the chunk-sum scan carries between rounds); windows of 2048 every 1024 rows
    start and end on chunk edges; 98 / 10 windows from row 5 of two recordings; 512 seeded windows, the first, the last and
    every window across row 262 144 are checked"""
    torch = torch_cuda
    rng, t, u, spk = _speaker(64, 16, salt=1)
    n = 300 * 1024 + 517
    mf = R.speaker_inputs(rng, n, 16)
    dev = torch.from_numpy(mf).cuda()
    edge = 256 * 1024
    for wf, hop, fo in ((2048, 1024, [0, n]), (98, 10, [5, 150001, n])):
        wins = R.scan_windows(fo, wf, hop)
        wo, sm, sl = spk.scan(dev, fo, wf, hop)
        assert int(wo[-1]) == len(wins)
        across = [w for w, (_r, s, c) in enumerate(wins) if s - fo[0] < edge <= s - fo[0] + c]
        assert across
        pick = sorted({0, len(wins) - 1} | set(across) | set(rng.choice(len(wins), size=min(512, len(wins)), replace=False).tolist()))
        rm, rl = R.speaker_scan(t, u, mf, fo, wf, hop, pick)
        assert np.array_equal(sm.cpu().numpy()[pick], rm) and np.array_equal(sl.cpu().numpy()[pick], rl), (wf, hop)


def test_speaker_scan_thousands_of_short_recordings(torch_cuda):
    """6000 recordings of 1-98 rows (one window each) and a few longer ones, from row 3: every window"""
    torch = torch_cuda
    rng, t, u, spk = _speaker(2, 7, salt=2)
    lens = rng.integers(1, 99, 6000)
    lens[rng.choice(6000, 20, replace=False)] = rng.integers(99, 400, 20)
    fo = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mf = np.zeros((int(fo[-1]), 7), F32)
    mf[3:] = R.speaker_inputs(rng, int(fo[-1]) - 3, 7)
    wo, sm, sl = spk.scan(torch.from_numpy(mf).cuda(), fo, 98, 10)
    assert int((np.diff(wo) == 1).sum()) >= 5000
    rm, rl = R.speaker_scan(t, u, mf, fo, 98, 10)
    assert np.array_equal(sm.cpu().numpy(), rm) and np.array_equal(sl.cpu().numpy(), rl)
