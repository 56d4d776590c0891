"""GPU: the scrub-jay RBF-SVM on seeded random models of every accepted shape, through every path, against the float64 reference of
tests/svm_ref.py (pinned to libsvm and the oracle by tests/test_svm_ref_cpu.py).

Paths: svm_kernel (SvmModel.predict), the POOL = 1 epilogue of the 512-point fused kernel (float, int16, ragged), the fused epilogue
of the 2048-point kernel (reference framing and aubio semantics), svm_scan_kernel (SvmModel.scan at tile widths 64 / 16 / 4 / 1 / 0,
ScrubJayScanner with head rows), and libsvm's tail (svm_binary_tail) that all of them share.  On every row of every path:
    decision  |dec_gpu - dec_ref| <= B, the reference's per-row bound of float32 evaluation in the kernels' orders;
    label     exactly the vote of the kernel's own decision (dec_gpu > 0 -> 0, else 1), and the reference's wherever |dec_ref| > B;
    P(1)      within 1e-6 of the float64 tail applied to dec_gpu -- or, where moving r01 by +-4 float32 ulps moves the iteration's
              stopping step, of one of those outcomes -- and always within 2.5e-7 of the nearest of them (the kernels' r01 is a
              float32 sigmoid: a few ulps from the double one; P carries one float32 rounding).
The fused and scan paths are checked on the pooled features they return (their `feat` output), with models fit to those features,
so that the check does not depend on the MFCC front end (gated elsewhere).  Each path's worst |err| / B and its accepted stopping-
test flips are printed as "SVM gate" lines."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import svm_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
P_TOL, P_NEAR = 1e-6, 2.5e-7
ULPS = 4
NO_CAP = 2**31 - 1
REPORT = {}

NF = [1, 2, 7, 8, 9, 26, 40, 63, 64, 65, 128, 255, 256]
NSV = [1, 2, 63, 64, 65, 128, 129, 2048, 2049, 5000]
GAMMA = [0.0, 1e-4, "1/nf", 0.025, 1.0, 50.0]
# two models per feature count: every n_sv and every gamma occurs, balanced and unbalanced dual coefficients
PREDICT = [(nf, NSV[(i + k * 5) % 10], GAMMA[(i + k * 3) % 6], k == 0) for i, nf in enumerate(NF) for k in (0, 1)]
FUSED512 = [(nm, [1, 64, 65, 2048][i % 4]) for i, nm in enumerate([1, 7, 8, 13, 16, 17, 20, 32])]
FUSED2048 = [(nm, nsv) for nm, nsv in zip([1, 13, 20, 32], [1, 65, 2049, 5000])]
SCAN_NF = [2, 26, 40, 64, 128]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for path in sorted(REPORT):
        worst, n, flips = REPORT[path]
        print(f"SVM gate {path:28s} rows {n:7d}  worst |err|/B {worst:.3f}  P(1) stopping-test flips accepted {flips}")


def _gamma(g, nf):
    return 1.0 / nf if g == "1/nf" else float(g)


def _check(path, attrs, feat, labels, dec, p1, what, far=None):
    """one path's outputs on rows feat against the reference (module docstring)"""
    ref = R.SvmRef(attrs)
    feat = np.asarray(feat, F32).reshape(-1, ref.nf)
    labels, dec, p1 = (np.asarray(a).reshape(-1) for a in (labels, dec, p1))
    assert labels.size == dec.size == p1.size == feat.shape[0], what
    rdec, bound = ref.decision(feat)
    dec64 = dec.astype(np.float64)
    ratio = np.abs(dec64 - rdec) / bound
    bad = ~(ratio <= 1.0)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: |dec - ref| = {abs(dec64[k] - rdec[k]):.3e} > B = {bound[k]:.3e} at row {k} (kernel {dec[k]!r}, "
                             f"reference {rdec[k]!r}); {int(bad.sum())} of {bad.size} rows miss")
    assert np.array_equal(labels, np.where(dec > 0, 0, 1)), f"{what}: label is not the vote of the kernel's own decision"
    firm = np.abs(rdec) > bound
    assert np.array_equal(labels[firm], np.where(rdec[firm] > 0, 0, 1)), f"{what}: label differs from the reference's"
    if far is not None:
        assert np.all(dec[far] == F32(np.ravel(attrs["rho"])[0])), f"{what}: rows where every K underflows must give rho exactly"
    outs, flip = R.tail_outcomes(dec64, ref.prob_a, ref.prob_b, ULPS)
    p = p1.astype(np.float64)
    base = np.abs(outs[:, ULPS] - p)
    near = np.abs(outs - p[:, None]).min(axis=1)
    ok = ((base <= P_TOL) | flip) & (near <= P_NEAR)
    if not ok.all():
        k = int(np.nonzero(~ok)[0][0])
        raise AssertionError(f"{what}: P(1) {p[k]!r} at row {k} (decision {dec[k]!r}): float64 tail {outs[k, ULPS]!r}, nearest "
                             f"+-{ULPS}-ulp outcome {near[k]:.3e} away, stopping step flips: {bool(flip[k])}; {int((~ok).sum())} rows miss")
    w, n, f = REPORT.get(path, (0.0, 0, 0))
    REPORT[path] = (max(w, float(ratio.max()) if ratio.size else 0.0), n + ratio.size, f + int((flip & (base > P_TOL)).sum()))
    return rdec, bound


def _dsp_einval(fn, match=None):
    from dsp_amd import lib as L
    with pytest.raises(L.DspError, match=r"failed \(-1\)") as e:
        fn()
    if match:
        assert match in str(e.value), str(e.value)
    return str(e.value)


def _noise(rng, lens):
    out = []
    for n in lens:
        x = rng.uniform(-1, 1, n).astype(F32)
        env = np.repeat(rng.uniform(0.002, 1.0, n // 1000 + 1).astype(F32), 1000)[:n]
        out.append((x * env).astype(F32))
    return out


def _ragged(torch, clips):
    off = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(clips)).cuda(), off


# ---- predict / three-kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf,n_sv,g,balanced", PREDICT)
def test_predict_random_models(torch_cuda, nf, n_sv, g, balanced):
    """SvmModel.predict (svm_kernel) on rows near SVs 0 / 63 / 64 / 65 / last and random ones, between SVs, and far from all of them"""
    torch = torch_cuda
    from dsp_amd import scrubjay
    rng = np.random.default_rng(nf * 100003 + n_sv * 7 + (0 if balanced else 1))
    attrs = R.random_svm(rng, nf, n_sv, _gamma(g, nf), balanced)
    x = R.probe_rows(rng, attrs)
    far = R.far_rows(attrs, x)
    assert far.any() == (_gamma(g, nf) > 0)
    svm = scrubjay.SvmModel(attrs)
    labels, dec, p1 = (a.cpu().numpy() for a in svm.predict(torch.from_numpy(x).cuda()))
    _check("predict", attrs, x, labels, dec, p1, f"predict nf {nf} n_sv {n_sv} gamma {g}", far)


def test_predict_refusals(torch_cuda):
    from dsp_amd import scrubjay
    rng = np.random.default_rng(3)
    _dsp_einval(lambda: scrubjay.SvmModel(R.random_svm(rng, 257, 3, 0.1)), "bad argument")
    a = R.random_svm(rng, 1, 3, 0.1)
    a.update(offset=np.zeros(0, F32), scale=np.zeros(0, F32), sv=np.zeros((3, 0), F32))
    _dsp_einval(lambda: scrubjay.SvmModel(a), "bad argument")


# ---- fused 512 ------------------------------------------------------------------------------------------------------------------

def _plan_features(torch, cfg, clips, max_frames=NO_CAP):
    """the three-kernel path's pooled features of equal-length clips (MFCC -> mfcc_stats)"""
    import dsp_amd
    from dsp_amd import scrubjay
    plan = dsp_amd.MfccPlan(cfg)
    return scrubjay.mfcc_stats(plan.clips(clips, max_frames)).cpu().numpy()


@pytest.mark.parametrize("n_mfcc,n_sv", FUSED512)
def test_fused512_float_and_ragged(torch_cuda, n_mfcc, n_sv):
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(5120 + 97 * n_mfcc + n_sv)
    cfg = dsp_amd.default_config(n_mfcc=n_mfcc)
    clips = torch.from_numpy(np.stack(_noise(rng, [8000] * 40))).cuda()
    attrs = R.svm_from_features(rng, _plan_features(torch, cfg, clips), n_sv)
    sj = scrubjay.ScrubJay(attrs, config=cfg)
    labels, dec, p1, feat = (a.cpu().numpy() for a in sj(clips))
    _check("fused512 float", attrs, feat, labels, dec, p1, f"fused 512 n_mfcc {n_mfcc} n_sv {n_sv}")
    sig, off = _ragged(torch, _noise(rng, rng.integers(400, 16000, 24).tolist()))
    pre = scrubjay.ScrubJay(R.random_svm(rng, 2 * n_mfcc, 1, 0.1), config=cfg).ragged(sig, off)[3].cpu().numpy()
    attrs = R.svm_from_features(rng, pre, n_sv)
    labels, dec, p1, feat = (a.cpu().numpy() for a in scrubjay.ScrubJay(attrs, config=cfg).ragged(sig, off))
    _check("fused512 ragged", attrs, feat, labels, dec, p1, f"fused 512 ragged n_mfcc {n_mfcc} n_sv {n_sv}")


# launch_mfcc512_pool expands every shape of DSP_FOR_SHAPES; default_config(n_mfcc=...) reaches (4,10,3) and (2,20,3) only.
# name -> (default_config overrides, (dct_split, dct_len, mel_gather) the plan must select)
FUSED512_SHAPES = {"mels41": (dict(n_mels=41, n_mfcc=13), (4, 16, 3)), "mels32": (dict(n_mels=32), (4, 10, 6)),
                   "mels17_mfcc17": (dict(n_mels=17, n_mfcc=17), (2, 20, 6))}


@pytest.mark.parametrize("which", list(FUSED512_SHAPES))
def test_fused512_other_instantiations(torch_cuda, which):
    """the clip -> label kernel on an LDS-resident DCT operand (4,16,3), on gather 6 (4,10,6) and on both with two coefficient
    tiles (2,20,6), against the two-step chain plan.clips -> mfcc_stats -> predict: its features, labels, decisions and P(1) are
    the chain's bit for bit (as tests/test_gpu_scrubjay.py holds for the default bank), and both are within the reference's bound"""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import lib as L
    from dsp_amd import scrubjay
    over, shape = FUSED512_SHAPES[which]
    cfg = dsp_amd.default_config(**over)
    t = L.LaneTables512()
    assert dsp_amd.load().dsp_mfcc_lane_tables(C.byref(cfg), C.byref(t), C.sizeof(t)) == 0
    assert (t.dct_split, t.dct_len, t.mel_gather) == shape and 2 * cfg.n_mfcc <= 64
    rng = np.random.default_rng(5120 + 131 * cfg.n_mels + cfg.n_mfcc)
    clips = torch.from_numpy(np.stack(_noise(rng, [8000] * 40))).cuda()
    attrs = R.svm_from_features(rng, _plan_features(torch, cfg, clips), 65)
    sj = scrubjay.ScrubJay(attrs, config=cfg)
    fused = [a.cpu().numpy() for a in sj(clips)]
    chain = [a.cpu().numpy() for a in sj(clips, fused=False)]
    for a, b, what in zip(fused, chain, ("labels", "decision", "P(1)", "features")):
        assert np.array_equal(a, b), f"fused 512 {which}: {what} differ from the two-step chain's"
    labels, dec, p1, feat = fused
    _check("fused512 shapes", attrs, feat, labels, dec, p1, f"fused 512 {which} {shape}")
    sig, off = _ragged(torch, _noise(rng, rng.integers(400, 16000, 24).tolist()))
    pre = scrubjay.ScrubJay(R.random_svm(rng, 2 * cfg.n_mfcc, 1, 0.1), config=cfg).ragged(sig, off)[3].cpu().numpy()
    attrs = R.svm_from_features(rng, pre, 65)
    sj = scrubjay.ScrubJay(attrs, config=cfg)
    labels, dec, p1, feat = (a.cpu().numpy() for a in sj.ragged(sig, off))
    _check("fused512 shapes ragged", attrs, feat, labels, dec, p1, f"fused 512 ragged {which} {shape}")
    for c in (0, 11, 23):                                    # and clip by clip against the chain
        one = [a.cpu().numpy() for a in sj(sig[off[c]:off[c + 1]].clone()[None], fused=False)]
        for a, b in zip((labels, dec, p1, feat), one):
            assert np.array_equal(a[c], b[0]), f"fused 512 ragged {which} clip {c}"


@pytest.mark.parametrize("n_mfcc", [13, 20])
def test_fused512_int16(torch_cuda, n_mfcc):
    """the two int16 shapes: mono, stereo channel 0, stereo average; equal-length and ragged batches"""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(1600 + n_mfcc)
    cfg = dsp_amd.default_config(n_mfcc=n_mfcc)
    pcm = np.stack([(c * 20000).astype(np.int16) for c in _noise(rng, [8000] * 24)])
    stereo = np.stack([pcm, np.roll(pcm, 3, axis=1)], axis=2)
    for i, (name, buf, mode) in enumerate((("mono", pcm, 0), ("stereo ch0", stereo, 0), ("stereo average", stereo, 1))):
        t = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
        pre = scrubjay.ScrubJay(R.random_svm(rng, 2 * n_mfcc, 1, 0.1), config=cfg).pcm16(t, stereo_mode=mode)[3].cpu().numpy()
        attrs = R.svm_from_features(rng, pre, [1, 65, 2048][i])
        sj = scrubjay.ScrubJay(attrs, config=cfg)
        labels, dec, p1, feat = (a.cpu().numpy() for a in sj.pcm16(t, stereo_mode=mode))
        _check("fused512 int16", attrs, feat, labels, dec, p1, f"fused 512 int16 {name} n_mfcc {n_mfcc}")
        flat = torch.from_numpy(np.ascontiguousarray(buf.reshape((-1,) + buf.shape[2:]))).cuda()
        off = np.arange(0, 8000 * 24 + 1, 8000, dtype=np.int64)
        labels, dec, p1, feat = (a.cpu().numpy() for a in sj.ragged(flat, off, stereo_mode=mode))
        _check("fused512 int16", attrs, feat, labels, dec, p1, f"fused 512 int16 ragged {name} n_mfcc {n_mfcc}")


def test_fused512_refuses_more_than_2048_svs(torch_cuda):
    """2049 support vectors do not fit the 512-point fused kernel's LDS: DSP_EINVAL naming the limit on the float, int16 and ragged
    entries, before anything runs; the same model runs on predict, the 2048-point fused paths and the scan"""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(2049)
    clips = torch.from_numpy(np.stack(_noise(rng, [16000] * 8))).cuda()
    cfg = dsp_amd.default_config(n_mfcc=13)
    attrs = R.svm_from_features(rng, _plan_features(torch, cfg, clips), 2049)
    sj = scrubjay.ScrubJay(attrs, config=cfg)
    pcm = (clips.cpu().numpy() * 20000).astype(np.int16)
    sig, off = _ragged(torch, _noise(rng, [4000, 9000]))
    for fn in (lambda: sj(clips), lambda: sj.pcm16(torch.from_numpy(pcm).cuda()), lambda: sj.ragged(sig, off),
               lambda: sj.ragged(torch.from_numpy(pcm.reshape(-1)).cuda(), np.arange(0, pcm.size + 1, 16000, dtype=np.int64))):
        assert "at most 2048 support vectors" in _dsp_einval(fn)
    labels, dec, p1, feat = (a.cpu().numpy() for a in sj(clips, fused=False))
    _check("predict", attrs, feat, labels, dec, p1, "2049 SVs on the three-kernel path")
    c2048 = scrubjay.scrubjay_infer_config(16000)
    c2048.n_mfcc = 13
    labels, dec, p1, feat = (a.cpu().numpy() for a in scrubjay.ScrubJay(attrs, config=c2048)(clips))
    _check("fused2048 aubio float", attrs, feat, labels, dec, p1, "2049 SVs on the 2048-point aubio path")
    mf = torch.from_numpy(rng.normal(0, 8, (300, 13)).astype(F32)).cuda()
    _wo, labels, dec, p1, feat = scrubjay.SvmModel(attrs).scan(mf, np.array([0, 300]), 16, 4)
    _check("scan", attrs, feat.cpu().numpy(), labels.cpu().numpy(), dec.cpu().numpy(), p1.cpu().numpy(), "2049 SVs on the scan")


# ---- fused 2048 -----------------------------------------------------------------------------------------------------------------

def _cfg2048(name, n_mfcc):
    from dsp_amd import scrubjay
    cfg = scrubjay.scrubjay_infer_config(16000, aubio=name == "aubio")
    cfg.n_mfcc = n_mfcc
    return cfg


@pytest.mark.parametrize("name", ["aubio", "reference"])
@pytest.mark.parametrize("n_mfcc,n_sv", FUSED2048)
def test_fused2048(torch_cuda, name, n_mfcc, n_sv):
    """float and ragged on both framings; int16 (mono, stereo, ragged) only under aubio semantics -- the reference framing refuses it"""
    torch = torch_cuda
    from dsp_amd import scrubjay
    rng = np.random.default_rng(20480 + 31 * n_mfcc + n_sv + (0 if name == "aubio" else 7))
    cfg = _cfg2048(name, n_mfcc)
    clips = torch.from_numpy(np.stack(_noise(rng, [16000] * 24))).cuda()
    attrs = R.svm_from_features(rng, _plan_features(torch, cfg, clips), n_sv)
    sj = scrubjay.ScrubJay(attrs, config=cfg)
    labels, dec, p1, feat = (a.cpu().numpy() for a in sj(clips))
    _check(f"fused2048 {name} float", attrs, feat, labels, dec, p1, f"fused 2048 {name} n_mfcc {n_mfcc} n_sv {n_sv}")
    sig, off = _ragged(torch, _noise(rng, rng.integers(2048, 40000, 16).tolist()))
    pre = scrubjay.ScrubJay(R.random_svm(rng, 2 * n_mfcc, 1, 0.1), config=cfg).ragged(sig, off)[3].cpu().numpy()
    attrs_r = R.svm_from_features(rng, pre, n_sv)
    labels, dec, p1, feat = (a.cpu().numpy() for a in scrubjay.ScrubJay(attrs_r, config=cfg).ragged(sig, off))
    _check(f"fused2048 {name} ragged", attrs_r, feat, labels, dec, p1, f"fused 2048 {name} ragged n_mfcc {n_mfcc} n_sv {n_sv}")
    pcm = (clips.cpu().numpy() * 20000).astype(np.int16)
    if name != "aubio":
        _dsp_einval(lambda: sj.pcm16(torch.from_numpy(pcm).cuda()), "int16 input")
        return
    stereo = np.ascontiguousarray(np.stack([pcm, np.roll(pcm, 5, axis=1)], axis=2))
    for tag, buf, mode in (("mono", pcm, 0), ("stereo average", stereo, 1)):
        t = torch.from_numpy(buf).cuda()
        pre = sj.pcm16(t, stereo_mode=mode)[3].cpu().numpy()
        attrs_p = R.svm_from_features(rng, pre, n_sv)
        sp = scrubjay.ScrubJay(attrs_p, config=cfg)
        labels, dec, p1, feat = (a.cpu().numpy() for a in sp.pcm16(t, stereo_mode=mode))
        _check("fused2048 aubio int16", attrs_p, feat, labels, dec, p1, f"fused 2048 int16 {tag} n_mfcc {n_mfcc}")
        flat = torch.from_numpy(np.ascontiguousarray(buf.reshape((-1,) + buf.shape[2:]))).cuda()
        labels, dec, p1, feat = (a.cpu().numpy() for a in sp.ragged(flat, np.arange(0, pcm.size + 1, 16000, dtype=np.int64), stereo_mode=mode))
        _check("fused2048 aubio int16", attrs_p, feat, labels, dec, p1, f"fused 2048 int16 ragged {tag} n_mfcc {n_mfcc}")


# ---- scans ----------------------------------------------------------------------------------------------------------------------

def _scan_lds(nf, wf, hop, tw):
    """svm_kernels.hip svm_scan_lds without head rows, bytes"""
    nc = nf // 2
    if tw == 0:
        return nf * 4
    return (tw * nf + ((tw - 1) * hop + wf) * nc) * 4


def _scan_tile(nf, wf, hop):
    for tw in (64, 16, 4, 1):
        if _scan_lds(nf, wf, hop, tw) <= 64 * 1024:
            return tw
    return 0


def _scan_shape(nf, tw):
    """the first (window, hop) of a fixed list that selects tile width tw for nf features"""
    for wf in (16, 33, 64, 98, 200, 400, 1000, 2000, 4000, 9000, 20000):
        for hop in (1, 3, 10, 40, 150, 400, 1000, 4000):
            if _scan_tile(nf, wf, hop) == tw:
                return wf, hop
    raise AssertionError((nf, tw))


@pytest.mark.parametrize("nf", SCAN_NF)
@pytest.mark.parametrize("tw", [64, 16, 4, 1, 0])
def test_scan_every_tile_width(torch_cuda, nf, tw):
    torch = torch_cuda
    from dsp_amd import scrubjay
    wf, hop = _scan_shape(nf, tw)
    rng = np.random.default_rng(nf * 1000 + tw)
    extra = min(2 * max(tw, 1) + 5, 70)
    lens = [1, max(1, wf - 1), wf, wf + hop * extra + 3]
    fo = 5 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mf = np.full((int(fo[-1]) + 3, nf // 2), np.nan, F32)
    mf[5:fo[-1]] = rng.normal(0, 8, (int(fo[-1]) - 5, nf // 2)) * rng.uniform(0.2, 2.0, (int(fo[-1]) - 5, 1))
    mft = torch.from_numpy(mf).cuda()
    pre = scrubjay.SvmModel(R.random_svm(rng, nf, 1, 0.1)).scan(mft, fo, wf, hop)[4].cpu().numpy()
    attrs = R.svm_from_features(rng, pre, [1, 65, 300, 2049][nf % 4])
    _wo, labels, dec, p1, feat = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in scrubjay.SvmModel(attrs).scan(mft, fo, wf, hop))
    assert np.isfinite(feat).all()
    _check("scan", attrs, feat, labels, dec, p1, f"scan nf {nf} ({wf}, {hop}) TW {tw}")


def _scan_c(svm, torch, nf_rows):
    """dsp_svm_scan_device called directly (SvmModel.scan refuses odd n_features in Python before the C ABI sees them)"""
    from dsp_amd import lib as L
    from dsp_amd.consumers import _scan_config
    mf = torch.zeros((40, max(1, nf_rows)), dtype=torch.float32, device="cuda")
    fo = np.array([0, 40], np.int64)
    out = [torch.empty(8, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32)] + \
          [torch.empty((8, 256), dtype=torch.float32, device="cuda")]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(svm._L.dsp_svm_scan_device(svm._h, mf.data_ptr(), 1, fo.ctypes.data_as(C.POINTER(C.c_long)), C.byref(_scan_config(40, 40)),
                                       *[t.data_ptr() for t in out], st), "dsp_svm_scan_device")


def test_scan_refusals(torch_cuda):
    from dsp_amd import scrubjay
    torch = torch_cuda
    rng = np.random.default_rng(130)
    for nf in (7, 65, 130):
        svm = scrubjay.SvmModel(R.random_svm(rng, nf, 3, 0.1))
        assert "n_features must be even, <= 128" in _dsp_einval(lambda: _scan_c(svm, torch, nf // 2))
    with pytest.raises(ValueError):
        scrubjay.SvmModel(R.random_svm(rng, 7, 3, 0.1)).scan(torch.zeros((40, 3), device="cuda"), [0, 40], 16, 4)


@pytest.mark.parametrize("name", ["512", "aubio"])
@pytest.mark.parametrize("wf,hf", [(16, 4), (98, 10)])
def test_scanner(torch_cuda, name, wf, hf):
    """ScrubJayScanner on the 512-point plan (20 coefficients) and the aubio plan (stream framing: windows with head rows)"""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(wf * 10 + hf + (0 if name == "512" else 1))
    cfg = dsp_amd.default_config(n_mfcc=20) if name == "512" else scrubjay.scrubjay_infer_config(16000)
    sig, off = _ragged(torch, _noise(rng, [16000, 400 * 16, 5 * 16000, 2048 * 3]))
    pre = scrubjay.ScrubJayScanner(scrubjay.ScrubJay(R.random_svm(rng, 40, 1, 0.1), config=cfg), wf, hf).run(sig, off)[4].cpu().numpy()
    attrs = R.svm_from_features(rng, pre, 300)
    sc = scrubjay.ScrubJayScanner(scrubjay.ScrubJay(attrs, config=cfg), wf, hf)
    _wo, labels, dec, p1, feat = sc.run(sig, off)
    _check(f"scanner {name}", attrs, feat.cpu().numpy(), labels.cpu().numpy(), dec.cpu().numpy(), p1.cpu().numpy(),
           f"scanner {name} ({wf}, {hf})")


# ---- libsvm's tail -------------------------------------------------------------------------------------------------------------

# (prob_a, prob_b): the golden model's, a positive slope, a steep one, and one whose branch changes sign far from d = 0
TAIL_AB = [(-2.2436, 0.0178), (1.0, 0.0), (-40.0, 0.3), (-0.05, 6.0)]


def _tail_decisions(a, b):
    """decision values d whose fApB = d a + b lands on each regime of the tail (float32)"""
    fs = [0.0, 1e-30, -1e-30, 1e-7, -1e-7, 16.0, -16.0, 88.0, -88.0, 104.0, -104.0, 120.0, -120.0]
    fs += [s * math.log(1.0 / R.R01_MIN - 1.0) * k for s in (1.0, -1.0) for k in (0.999, 1.0, 1.001)]     # r01 at the clamps
    r01 = list(R.stop_boundaries(n=100001)) + list(np.linspace(0.485, 0.515, 25))                          # stopping boundaries, dead zone
    fs += [math.log(1.0 / r - 1.0) for r in r01]
    ds = []
    for f in fs:
        d = F32((f - b) / a)
        ds += [d, np.nextafter(d, F32(np.inf)), np.nextafter(d, F32(-np.inf))]
    d0 = F32(-b / a)                                                                                       # fApB's sign change
    ds += [d0] + [F32(d0 + k * np.spacing(d0)) for k in (-3, -2, -1, 1, 2, 3)]
    ds += [F32(0.0), F32(1e-30), F32(-1e-30)]
    return np.unique(np.array(ds, F32))


def test_tail_sweep(torch_cuda):
    """gamma = 0, one SV, coef = d, rho = 0: every path's decision is d exactly, whatever its input; the label and P(1) must then be
    libsvm's on d (vote at d = 0 -> 1, clamps, expf overflow / underflow of fApB, the iteration's dead zone and stopping steps),
    through predict, fused 512, fused 2048 and the scan"""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(77)
    nm, nf = 13, 26
    x = torch.from_numpy(rng.normal(0, 3, (3, nf)).astype(F32)).cuda()
    clips512 = torch.from_numpy(np.stack(_noise(rng, [4000] * 2))).cuda()
    clips2048 = torch.from_numpy(np.stack(_noise(rng, [8192] * 2))).cuda()
    mf = torch.from_numpy(rng.normal(0, 8, (40, nm)).astype(F32)).cuda()
    base = R.random_svm(rng, nf, 1, 0.0)
    s512 = scrubjay.ScrubJay(base, config=dsp_amd.default_config(n_mfcc=nm))
    s2048 = scrubjay.ScrubJay(base, config=_cfg2048("aubio", nm))
    got = {k: [] for k in ("predict", "fused512", "fused2048", "scan")}
    for a, b in TAIL_AB:
        for d in _tail_decisions(a, b):
            attrs = dict(base, coef=np.array([d], F32), rho=np.array([0.0], F32), prob_a=np.array([a], F32), prob_b=np.array([b], F32))
            svm = scrubjay.SvmModel(attrs)
            s512.svm = s2048.svm = svm
            outs = {"predict": svm.predict(x), "fused512": s512(clips512)[:3], "fused2048": s2048(clips2048)[:3],
                    "scan": svm.scan(mf, np.array([0, 40]), 16, 8)[1:4]}
            for k, (lab, dec, p1) in outs.items():
                got[k].append((attrs, d, lab.cpu().numpy(), dec.cpu().numpy(), p1.cpu().numpy()))
    for path, rows in got.items():
        flips = 0
        for attrs, d, lab, dec, p1 in rows:
            assert np.all(dec == d), (path, d, dec)
            assert np.array_equal(lab, np.full(lab.shape, 0 if d > 0 else 1)), (path, d, lab)
            ra, rb = float(attrs["prob_a"][0]), float(attrs["prob_b"][0])
            outs, flip = R.tail_outcomes(dec.astype(np.float64), ra, rb, ULPS)
            p = p1.astype(np.float64)
            basev = np.abs(outs[:, ULPS] - p)
            near = np.abs(outs - p[:, None]).min(axis=1)
            assert np.all(((basev <= P_TOL) | flip) & (near <= P_NEAR)), (path, d, ra, rb, p, outs[:, ULPS], flip)
            flips += int((flip & (basev > P_TOL)).sum())
        w, n, f = REPORT.get(f"tail {path}", (0.0, 0, 0))
        REPORT[f"tail {path}"] = (0.0, n + len(rows), f + flips)
    zero = [r for r in got["predict"] if r[1] == 0.0]
    assert zero and all(np.all(r[2] == 1) for r in zero)
