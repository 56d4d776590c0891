"""Plain numpy references of the MFCC consumers, no GPU and no library: the stop-word net and the speaker GMM LLR, for any model
the C ABI accepts.  tests/test_consumer_ref_cpu.py pins them against the oracle; tests/test_gpu_consumer_models.py holds every
device path to them.

Stop net (stop_detector.c:26-50, audio_classifier_inference.c:18-90): the input is standardised in float32 exactly as the
reference does it, xs = fl32(fl32(x - mean) / div) with div = scale, 0 replaced by 1.  Layer 1 is summed EXACTLY (math.fsum over
the float64 products, which are exact) and rounded to float32 once; the reference's own sequential float32 sum sits within 2e-5
of it.  Layers 2-4 run in float32 in the reference's order, s = s + w * h (two roundings, no FMA), then the sigmoid.

Speaker GMM (speaker_gmm.c:29-141): exact integers.  x Q6 = (int16)(int32)(x * 64), truncation then the low 16 bits; per mixture
sum_d (x - mean)^2 inv_cov, >> 15 (arithmetic), / 2 (toward zero), log_const minus that, max over mixtures; per row LL_target -
LL_ubm; per clip or window the truncating mean.  The domain is asserted, not assumed: |x * 64| < 2^31 and no intermediate outside
int64.  A draw outside it is a bug of the test that drew it."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
SPEAKER_THRESHOLD = int(-0.7 * (1 << 8))           # speaker_gmm.c:124-125: -179
_I63 = 1 << 63


# ---- stop-word net -----------------------------------------------------------------------------------------------------------

class StopNet:
    """One stop model's parameters in the reference's layout (the same dict StopModel / oracle.stop_predict take)."""

    def __init__(self, model: dict):
        self.n_coef, self.max_frames = int(model.get("n_coef", 13)), int(model.get("max_frames", 500))
        n_in = self.n_coef * self.max_frames
        self.mean = np.asarray(model["scaler_mean"], F32).reshape(n_in)
        scale = np.asarray(model["scaler_scale"], F32).reshape(n_in)
        self.div = np.where(scale == 0.0, F32(1.0), scale).astype(F32)            # audio_classifier_inference.c:44-45
        self.units = [int(np.asarray(model[f"bias{i}"]).size) for i in range(4)]
        fan, self.w, self.b = n_in, [], []
        for i, u in enumerate(self.units):
            self.w.append(np.asarray(model[f"kernel{i}"], F32).reshape(fan, u))
            self.b.append(np.asarray(model[f"bias{i}"], F32).reshape(u))
            fan = u
        self._w1 = self.w[0].astype(np.float64)
        self._pad = {}
        # first-order propagation of a relative error e of every layer-1 term to P: e * sum|w xs| * prod ||W_l||_inf / 4
        self._gain = math.prod(float(np.abs(w).sum(axis=0).max()) for w in self.w[1:]) / 4.0

    def standardise(self, feats: np.ndarray) -> np.ndarray:
        """xs = fl32(fl32(x - mean) / div) of coefficient-major feature vectors [..., n_coef * max_frames]"""
        return ((np.asarray(feats, F32) - self.mean).astype(F32) / self.div).astype(F32)

    def _pad_partials(self, tc: int):
        """per unit, non-overlapping float64 partials whose exact sum is the zero-padded frames' (t >= tc) layer-1 terms"""
        if tc not in self._pad:
            idx = (np.arange(self.n_coef)[:, None] * self.max_frames + np.arange(tc, self.max_frames)[None, :]).reshape(-1)
            xs = ((F32(0.0) - self.mean[idx]).astype(F32) / self.div[idx]).astype(F32)
            prods = self._w1[idx] * xs.astype(np.float64)[:, None]                  # exact: float32 x float32 fits a float64
            self._pad[tc] = ([_msum(prods[:, j].tolist()) for j in range(self.units[0])], np.abs(prods).sum(axis=0))
        return self._pad[tc]

    def _tail(self, s1: np.ndarray) -> F32:
        h = np.maximum(s1.astype(F32), F32(0.0))
        for l in (1, 2, 3):                                                          # dense_forward, :18-35
            w, b = self.w[l], self.b[l]
            out = np.empty(self.units[l], F32)
            for j in range(self.units[l]):
                s = b[j]
                for i in range(h.size):
                    s = F32(s + F32(w[i, j] * h[i]))
                out[j] = s if l == 3 or s > F32(0.0) else F32(0.0)
            h = out
        return F32(F32(1.0) / (F32(1.0) + np.exp(-h[0])))                           # :13-15

    def prob(self, mfcc: np.ndarray):
        """classify_signal's net on one frame-major MFCC matrix [T][n_coef] (T clamped to max_frames, zero padded)
        -> (P float32, first-order bound of a 2^-22 relative error per layer-1 term)"""
        mfcc = np.asarray(mfcc, F32).reshape(-1, self.n_coef)
        tc = min(mfcc.shape[0], self.max_frames)                                     # stop_detector.c:26-30
        idx = (np.arange(self.n_coef)[None, :] * self.max_frames + np.arange(tc)[:, None]).reshape(-1)   # frame-major -> i = c max + t
        xs = ((mfcc[:tc].reshape(-1) - self.mean[idx]).astype(F32) / self.div[idx]).astype(F32)
        prods = self._w1[idx] * xs.astype(np.float64)[:, None]
        pad, pad_abs = self._pad_partials(tc)
        s1 = np.array([math.fsum(prods[:, j].tolist() + pad[j] + [float(self.b[0][j])]) for j in range(self.units[0])])
        bound = 2.0 ** -22 * float((np.abs(prods).sum(axis=0) + pad_abs).max()) * self._gain
        return self._tail(s1), bound

    def prob_feats(self, feats: np.ndarray) -> F32:
        """the net on one coefficient-major feature vector (stop_features' layout: every input, padding included)"""
        xs = self.standardise(np.asarray(feats, F32).reshape(-1)).astype(np.float64)
        prods = self._w1 * xs[:, None]
        return self._tail(np.array([math.fsum(prods[:, j].tolist() + [float(self.b[0][j])]) for j in range(self.units[0])]))

    def layer1_estimate(self, mfccs) -> np.ndarray:
        """float64 layer-1 sums without the bias, [len(mfccs)][units[0]]: a quick estimate for drawing biases, not a reference"""
        out = np.empty((len(mfccs), self.units[0]))
        for k, m in enumerate(mfccs):
            feats = np.zeros((self.n_coef, self.max_frames), F32)
            m = np.asarray(m, F32).reshape(-1, self.n_coef)[:self.max_frames]
            feats[:, :m.shape[0]] = m.T
            out[k] = self.standardise(feats.reshape(-1)).astype(np.float64) @ self._w1
        return out


def _msum(xs):
    """Shewchuk's exact summation: non-overlapping float64 partials whose exact sum is sum(xs) (finite inputs, no overflow)"""
    partials = []
    for x in xs:
        i = 0
        for y in partials:
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                partials[i] = lo
                i += 1
            x = hi
        partials[i:] = [x]
    return partials


def scan_windows(frame_offsets, window_frames: int, hop_frames: int):
    """the window rule of a ragged MFCC matrix: per window (recording, first row, rows).  Window w of a recording of R >=
    window_frames rows is rows [w hop, w hop + window_frames); a recording with fewer rows has one window of all of them."""
    fo = np.asarray(frame_offsets, np.int64)
    out = []
    for r in range(fo.size - 1):
        n = int(fo[r + 1] - fo[r])
        if n < window_frames:
            out.append((r, int(fo[r]), n))
        else:
            out.extend((r, int(fo[r]) + w * hop_frames, window_frames) for w in range(1 + (n - window_frames) // hop_frames))
    return out


def stop_scan(net: StopNet, mfcc: np.ndarray, frame_offsets, window_frames: int, hop_frames: int, pick=None):
    """P("stop") and its bound for every window of the ragged matrix mfcc [F][n_coef] (or the windows `pick` indexes)
    -> (prob float32 [n], bound float64 [n])"""
    wins = scan_windows(frame_offsets, window_frames, hop_frames)
    sel = range(len(wins)) if pick is None else pick
    res = [net.prob(mfcc[s:s + n]) for (_r, s, n) in (wins[i] for i in sel)]
    return np.array([p for p, _b in res], F32), np.array([b for _p, b in res])


def stop_scan_tile(n_coef: int, max_frames: int, u1: int, window_frames: int, hop_frames: int) -> int:
    """windows per block the scan kernel uses (consumer_kernels.hip stop_scan_tile): the widest tile in (64, 16, 4, 1) whose
    staged rows (or float64 partial sums) fit 64 KiB of LDS, 0 when none does"""
    ln = min(window_frames, max_frames)
    for tw in (64, 16, 4, 1):
        if max(((tw - 1) * hop_frames + ln) * n_coef * 4, 256 * u1 * 8) <= 64 * 1024:
            return tw
    return 0


# ---- speaker GMM -------------------------------------------------------------------------------------------------------------

def q6(x: np.ndarray) -> np.ndarray:
    """(int16)(int32)(x * 64) as int64: x * 64 in float32, truncated toward zero, the low 16 bits as a signed value"""
    v = np.asarray(x, F32) * F32(64.0)
    assert np.all(np.isfinite(v)) and np.all(np.abs(v.astype(np.float64)) < 2.0 ** 31), "Q6 input outside |x * 64| < 2^31"
    t = np.trunc(v).astype(np.int64)
    return ((t + 32768) & 0xFFFF) - 32768


def _tdiv(a: np.ndarray, n) -> np.ndarray:
    """C's int64 division (toward zero) of a by n > 0"""
    return np.where(a < 0, -((-a) // n), a // n)


def gmm_ll(g: dict, xq: np.ndarray) -> np.ndarray:
    """per row of Q6 inputs xq [N][D]: max over mixtures of log_const - ((sum_d (x - mean)^2 inv_cov) >> 15) / 2 -> int64 [N]"""
    means = np.asarray(g["means"], np.int64)
    ic = np.asarray(g["inv_covs"], np.int64)
    lc = np.asarray(g["log_consts"], np.int64)
    xq = np.asarray(xq, np.int64)
    k, d = means.shape
    assert xq.ndim == 2 and xq.shape[1] == d
    if xq.shape[0] == 0:
        return np.zeros(0, np.int64)
    # domain: the largest |partial sum| any row can reach, in Python integers, below 2^63
    lo, hi = xq.min(axis=0).tolist(), xq.max(axis=0).tolist()
    worst = max(sum(max(abs(lo[j] - int(means[m, j])), abs(hi[j] - int(means[m, j]))) ** 2 * abs(int(ic[m, j])) for j in range(d))
                for m in range(k))
    assert worst < _I63, "GMM draw leaves int64"
    out = np.empty(xq.shape[0], np.int64)
    step = max(1, (1 << 22) // (k * d))
    for a in range(0, xq.shape[0], step):
        diff = xq[a:a + step, None, :] - means[None]
        sq = (diff * diff * ic[None]).sum(axis=2)
        out[a:a + step] = (lc[None] - _tdiv(sq >> 15, 2)).max(axis=1)
    return out


def speaker_rows(target: dict, ubm: dict, mfcc: np.ndarray):
    """per row of mfcc [N][D]: (LL_target, LL_ubm) int64 [N] each"""
    xq = q6(np.asarray(mfcc, F32).reshape(-1, np.asarray(target["means"]).shape[1]))
    return gmm_ll(target, xq), gmm_ll(ubm, xq)


def _window_means(v: np.ndarray, starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    assert float(np.abs(v.astype(np.float64)).sum()) < 2.0 ** 62, "LLR sums leave int64"
    q = np.concatenate([[0], np.cumsum(v)])
    return _tdiv(q[starts + lens] - q[starts], lens)


def speaker_means(target: dict, ubm: dict, mfcc: np.ndarray, frame_offsets):
    """mfcc_target_speaker_llr_mean per clip of a ragged matrix (every clip >= 1 row) -> (llr_mean int64 [n], label int32 [n])"""
    fo = np.asarray(frame_offsets, np.int64)
    assert (np.diff(fo) > 0).all()
    lt, lu = speaker_rows(target, ubm, mfcc[fo[0]:fo[-1]])
    m = _window_means(lt - lu, fo[:-1] - fo[0], np.diff(fo))
    return m, (m > SPEAKER_THRESHOLD).astype(np.int32)


def speaker_scan(target: dict, ubm: dict, mfcc: np.ndarray, frame_offsets, window_frames: int, hop_frames: int, pick=None):
    """the LLR mean and label of every window of a ragged matrix (or the windows `pick` indexes); the rows are scored in chunks
    -> (llr_mean int64 [n], label int32 [n])"""
    fo = np.asarray(frame_offsets, np.int64)
    wins = scan_windows(fo, window_frames, hop_frames)
    sel = np.arange(len(wins)) if pick is None else np.asarray(pick, np.int64)
    starts = np.array([wins[i][1] for i in sel], np.int64) - fo[0]
    lens = np.array([wins[i][2] for i in sel], np.int64)
    assert (lens > 0).all()
    rows = mfcc[fo[0]:fo[-1]]
    v = np.empty(rows.shape[0], np.int64)
    for a in range(0, rows.shape[0], 1 << 16):
        lt, lu = speaker_rows(target, ubm, rows[a:a + (1 << 16)])
        v[a:a + lt.size] = lt - lu
    m = _window_means(v, starts, lens)
    return m, (m > SPEAKER_THRESHOLD).astype(np.int32)


# ---- seeded model draws (shared by the CPU and GPU tests) ----------------------------------------------------------------------

def stop_data_shape(rng, n_coef: int):
    """(loc, spread) per coefficient of synthetic MFCC rows: spreads of 0.1 .. 10, and on about a third of the coefficients (always
    coefficient 0) an offset of 10 .. 500 spreads -- where a scaler fit to the data has |mean| / scale up to about 1e3"""
    spread = 10.0 ** rng.uniform(-1.0, 1.0, n_coef)
    loc = spread * rng.standard_normal(n_coef)
    big = rng.random(n_coef) < 1 / 3
    big[0] = True
    loc[big] = spread[big] * rng.choice([-1.0, 1.0], int(big.sum())) * 10.0 ** rng.uniform(1.0, 2.7, int(big.sum()))
    return loc, spread


def stop_rows(rng, shape, n_rows: int) -> np.ndarray:
    """n_rows synthetic MFCC rows of the data shape (loc, spread)"""
    loc, spread = shape
    return (loc + spread * rng.standard_normal((n_rows, loc.size))).astype(F32)


def random_stop_model(rng, n_coef: int, max_frames: int, units, loc=None, spread=None) -> dict:
    """A stop model for data whose coefficient c is about loc[c] +- spread[c] (default 0 +- 1): a StandardScaler near that data
    (so |mean| / scale is as large as the data's offset makes it), with every 17th scale 0 (the reference's guard) and a few
    scales near 1e-6 (their weight rows shrink with them, as a trained net's would); weights N(0, 1) / sqrt(fan_in).  Biases are
    zero: set them with fit_biases() for the inputs at hand."""
    units = tuple(int(u) for u in units)
    n_in = n_coef * max_frames
    loc = np.zeros(n_coef) if loc is None else np.asarray(loc, np.float64)
    spread = np.ones(n_coef) if spread is None else np.asarray(spread, np.float64)
    c = np.repeat(np.arange(n_coef), max_frames)                          # input i = c * max_frames + t
    scale = spread[c] * rng.uniform(0.5, 2.0, n_in)
    mean = loc[c] + spread[c] * rng.normal(0.0, 0.3, n_in)
    w0 = rng.standard_normal((n_in, units[0])) / math.sqrt(n_in)
    tiny = rng.choice(n_in, size=min(n_in, 3), replace=False)
    scale[tiny] = rng.uniform(0.8e-6, 1.5e-6, tiny.size)
    mean[tiny] = loc[c[tiny]] + scale[tiny] * rng.normal(0.0, 1.0, tiny.size)
    w0[tiny] *= scale[tiny, None] / spread[c[tiny], None]
    scale[::17] = 0.0
    m = {"n_coef": n_coef, "max_frames": max_frames, "scaler_mean": mean.astype(F32), "scaler_scale": scale.astype(F32),
         "kernel0": w0.astype(F32).reshape(-1), "bias0": np.zeros(units[0], F32)}
    fan = units[0]
    for i, u in enumerate(units[1:], start=1):
        m[f"kernel{i}"] = (rng.standard_normal((fan, u)) / math.sqrt(fan)).astype(F32).reshape(-1)
        m[f"bias{i}"] = np.zeros(u, F32)
        fan = u
    return m


def fit_biases(rng, model: dict, mfccs) -> dict:
    """Biases drawn for the inputs at hand so that the net's probabilities spread over (0, 1) instead of sitting on a plateau:
    each layer's bias puts about 70% of its units' pre-activations above zero, and the logit is centred and scaled to about
    +-3.  Float64 estimates; the reference is evaluated afterwards on the model as returned."""
    m = dict(model)
    net = StopNet(m)
    z = net.layer1_estimate(mfccs)
    m["bias0"] = (-np.quantile(z, 0.3, axis=0)).astype(F32)
    h = np.maximum(z + m["bias0"], 0.0)
    for l in (1, 2):
        z = h @ net.w[l].astype(np.float64)
        m[f"bias{l}"] = (-np.quantile(z, 0.3, axis=0) + 1e-3 * rng.standard_normal(z.shape[1])).astype(F32)
        h = np.maximum(z + m[f"bias{l}"], 0.0)
    z = (h @ net.w[3].astype(np.float64))[:, 0]
    sd = float(z.std())
    gain = 3.0 / sd if sd > 0 else 1.0
    m["kernel3"] = (net.w[3] * gain).astype(F32).reshape(-1)
    m["bias3"] = np.array([-np.median(z) * gain + 0.2 * rng.standard_normal()], F32)
    return m


def random_gmm(rng, k: int, d: int) -> dict:
    """A GMM over the full int8 means and int16 log-consts; inverse covariances of per-mixture magnitude 2^0 .. 2^28 (some
    negative, a few zero), so sum_d diff^2 |inv_cov| < 16 * 32895^2 * 2^28 < 2^63 for any Q6 input."""
    mag = 2.0 ** rng.uniform(0.0, 28.0, (k, 1))
    ic = np.round(mag * rng.uniform(0.0, 1.0, (k, d))).astype(np.int64)
    ic[rng.random((k, d)) < 0.1] *= -1
    ic[rng.random((k, d)) < 0.05] = 0
    ic = np.clip(ic, -(1 << 28), 1 << 28)
    return {"means": rng.integers(-128, 128, (k, d)).astype(np.int8), "inv_covs": ic.astype(np.int32),
            "log_consts": rng.integers(-32768, 32768, k).astype(np.int16)}


# x * 64 on the Q6 edges: just inside and at the int16 range, past it (wraps), a negative fraction, negative zero
Q6_EDGES = np.array([32767.5, 32767.0, -32767.5, -32768.0, 32768.0, -32768.9, 65535.0, 65536.0 + 0.5, -0.99, -0.0, 0.99, 1.0],
                    np.float64) / 64.0


def speaker_inputs(rng, n_rows: int, d: int, edges: bool = True) -> np.ndarray:
    """MFCC-like rows (+-20, Q6 +-1280) with, when edges, about 3% of entries on the Q6 edges"""
    x = (rng.standard_normal((n_rows, d)) * 8.0).astype(F32)
    if edges:
        hit = rng.random((n_rows, d)) < 0.03
        x[hit] = rng.choice(Q6_EDGES, int(hit.sum())).astype(F32)
    return x
