"""Plain numpy reference of the scrub-jay RBF-SVM, no GPU and no library: decision value, a per-row bound on what float32
evaluation may cost, and libsvm's two-class label and probability tail, for any model the C ABI accepts.
tests/test_svm_ref_cpu.py pins it against libsvm and the oracle; tests/test_gpu_svm_models.py holds every device path to it.

Decision (ONNX Scaler -> SVMClassifier, RBF, two classes).  The Scaler is part of the definition and runs in float32 exactly as the
ONNX operator and every kernel do it, z = fl32(fl32(x - offset) * scale).  Everything after it is float64 on the model's float32
parameters: d2_i = sum_j (z_j - sv_ij)^2, K_i = exp(-gamma d2_i), dec = sum_i coef_i K_i + rho.

Bound.  The kernels (svm_kernel, the fused 512- and 2048-point epilogues, svm_scan_kernel) evaluate, in float32 with no FMA:
    d_j = fl(z_j - sv_ij)                      relative error u (z and sv are float32: one rounding)
    d2 = sum_j fl(d_j d_j), left to right      |d2^ - d2| <= (nf + 3) u d2       (two roundings per square, nf - 1 additions)
    t = fl(-gamma d2^), K^ = expf(t)           relative u and ~2 ulp of expf -> |K^ - K| <= K (gamma (nf + 4) u d2 + 3 u)
    fl(coef K^)                                relative u
    lane sums of ceil(n_sv / 64) terms         each term carried through at most ceil(n_sv / 64) additions
    a 6-level xor butterfly, + rho             6 more additions of partial sums bounded by sum_i |coef_i| K_i, and u |dec|
which, to first order (u = 2^-24, gamma (nf + 4) u d2 <= 104 (nf + 4) u < 2e-3 wherever K is not below float32's range), is
    B = c u ( sum_i |coef_i| K_i (gamma (nf + 9) d2_i + ceil(n_sv / 64) + 12) + |dec| ) + 2^-125 sum_i |coef_i|
with the safety factor c = 2; the last term covers K_i or coef_i K_i in or below float32's subnormal range.  A looser scale such as
E_i = sum_j (|z_j| + |sv_ij|)^2 is not needed: the subtraction of two float32 values errs by u of its own result, so d2_i itself
is the scale of the distance error.  `terms` replaces ceil(n_sv / 64) for evaluations in another order (the oracle's sequential sum: n_sv).

Tail (libsvm svm.cpp: svm_predict, sigmoid_predict, multiclass_probability with k = 2), in double: label = 0 if dec > 0 else 1
(the vote); r01 = sigmoid_predict(dec, A, B) clamped to [1e-7, 1 - 1e-7]; p = multiclass_probability's iteration from (1/2, 1/2)
with tolerance 0.005 / 2 and at most 100 steps; P(label 1) = p[1]."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
SAFETY = 2.0
R01_MIN = 1e-7


class SvmRef:
    """One SVM's attributes (the dict SvmModel takes: offset, scale, sv, coef, kernel_params, rho, prob_a, prob_b)."""

    def __init__(self, attrs: dict):
        self.offset = np.ascontiguousarray(attrs["offset"], F32).reshape(-1)
        self.scale = np.ascontiguousarray(attrs["scale"], F32).reshape(-1)
        self.nf = self.offset.size
        self.sv = np.ascontiguousarray(attrs["sv"], F32).reshape(-1, self.nf)
        self.coef = np.ascontiguousarray(attrs["coef"], F32).reshape(-1)
        self.n_sv = self.coef.size
        assert self.sv.shape[0] == self.n_sv
        self.gamma = float(F32(np.ravel(attrs["kernel_params"])[0]))
        self.rho = float(F32(np.ravel(attrs["rho"])[0]))
        self.prob_a = float(F32(np.ravel(attrs["prob_a"])[0]))
        self.prob_b = float(F32(np.ravel(attrs["prob_b"])[0]))
        self._sv64 = self.sv.astype(np.float64)
        self._c64 = self.coef.astype(np.float64)

    def standardise(self, x) -> np.ndarray:
        """the ONNX Scaler in float32: fl32(fl32(x - offset) * scale)"""
        x = np.asarray(x, F32).reshape(-1, self.nf)
        return ((x - self.offset).astype(F32) * self.scale).astype(F32)

    def decision(self, x, terms: int | None = None):
        """rows x [N][nf] (float32 features) -> (dec float64 [N], bound B float64 [N]); the float64 work is chunked (<= ~32 MB)"""
        z = self.standardise(x).astype(np.float64)
        n = z.shape[0]
        dec, bound = np.empty(n), np.empty(n)
        terms = math.ceil(self.n_sv / 64) if terms is None else int(terms)
        step = max(1, (1 << 22) // max(1, self.n_sv * self.nf))
        for a in range(0, n, step):
            d2 = np.empty((min(step, n - a), self.n_sv))
            for k in range(d2.shape[0]):
                diff = z[a + k][None, :] - self._sv64
                d2[k] = np.einsum("ij,ij->i", diff, diff)
            kv = np.exp(-self.gamma * d2)
            ck = self._c64[None, :] * kv
            dec[a:a + d2.shape[0]] = ck.sum(axis=1) + self.rho
            amp = np.abs(ck) * (self.gamma * (self.nf + 9) * d2 + terms + 12)
            bound[a:a + d2.shape[0]] = amp.sum(axis=1)
        bound = SAFETY * U * (bound + np.abs(dec)) + 2.0 ** -125 * float(np.abs(self._c64).sum())
        return dec, bound

    def predict(self, x):
        """-> (label int32 [N], dec, B, p1 float64 [N]): the reference's answer for rows x"""
        dec, bound = self.decision(x)
        label, p1 = tail(dec, self.prob_a, self.prob_b)
        return label, dec, bound, p1


def sigmoid_r01(dec, prob_a: float, prob_b: float) -> np.ndarray:
    """libsvm's sigmoid_predict in double, clamped to [1e-7, 1 - 1e-7] (svm_predict_probability)"""
    return _sigmoid(np.asarray(dec, np.float64) * prob_a + prob_b)


def _sigmoid(f) -> np.ndarray:
    e = np.exp(-np.abs(f))                                                   # exp(-fApB) for fApB >= 0, exp(fApB) below
    return np.clip(np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e)), R01_MIN, 1.0 - R01_MIN)


def multiclass_p1(r01) -> tuple[np.ndarray, np.ndarray]:
    """libsvm's multiclass_probability for k = 2 on r[0][1] = r01, r[1][0] = 1 - r01, vectorised over r01 (float64)
    -> (p[1], the step at which the iteration stopped)"""
    r01 = np.asarray(r01, np.float64)
    r10 = 1.0 - r01
    q00, q11, q01 = r10 * r10, r01 * r01, -r10 * r01
    p0, p1 = np.full(r01.shape, 0.5), np.full(r01.shape, 0.5)
    steps = np.full(r01.shape, 100, np.int64)
    live = np.ones(r01.shape, bool)
    eps = 0.005 / 2
    for it in range(100):
        qp0, qp1 = q00 * p0 + q01 * p1, q01 * p0 + q11 * p1
        pqp = p0 * qp0 + p1 * qp1
        err = np.maximum(np.abs(qp0 - pqp), np.abs(qp1 - pqp))
        stop = live & (err < eps)
        steps[stop] = it
        live &= ~stop
        if not live.any():
            break
        # t = 0
        diff = (-qp0 + pqp) / q00
        n0 = p0 + diff
        npqp = (pqp + diff * (diff * q00 + 2 * qp0)) / (1 + diff) / (1 + diff)
        nqp0, nqp1 = (qp0 + diff * q00) / (1 + diff), (qp1 + diff * q01) / (1 + diff)
        n0, n1 = n0 / (1 + diff), p1 / (1 + diff)
        # t = 1
        diff = (-nqp1 + npqp) / q11
        n1 = n1 + diff
        n0, n1 = n0 / (1 + diff), n1 / (1 + diff)
        p0, p1 = np.where(live, n0, p0), np.where(live, n1, p1)
    return p1, steps


def tail(dec, prob_a: float, prob_b: float):
    """-> (vote label int32, P(label 1) float64) of decision values dec"""
    dec = np.asarray(dec, np.float64)
    p1, _steps = multiclass_p1(sigmoid_r01(dec, prob_a, prob_b))
    return np.where(dec > 0, 0, 1).astype(np.int32), p1


def tail_outcomes(dec, prob_a: float, prob_b: float, ulps: int = 4):
    """P(label 1) for r01 moved by -ulps .. +ulps float32 ulps around its double value and around its value from a float32 fApB
    -> (p1 [N][2 (2 ulps + 1)] (column `ulps` is tail()'s), stopping step differs among them [N] bool).  A float32 sigmoid lands
    within a few ulps of the double one; where that moves the iteration's stopping step, every one of these outcomes is right."""
    dec = np.asarray(dec, np.float64)
    r = sigmoid_r01(dec, prob_a, prob_b)
    # the kernels form fApB = dec A + B in float32: where that rounding moves r01 by more than a few ulps (|dec A| ~ |B| >> |fApB|),
    # r01 of the float32 fApB is the other centre
    r32 = _sigmoid((dec.astype(F32) * F32(prob_a) + F32(prob_b)).astype(np.float64))
    cols, steps = [], []
    for c in (r, r32):
        ulp = np.spacing(np.abs(c).astype(F32)).astype(np.float64)
        for k in range(-ulps, ulps + 1):
            p, s = multiclass_p1(np.clip(c + k * ulp, R01_MIN, 1.0 - R01_MIN))
            cols.append(p)
            steps.append(s)
    steps = np.stack(steps, axis=1)
    return np.stack(cols, axis=1), (steps != steps[:, :1]).any(axis=1)


def stop_boundaries(lo: float = 1e-6, hi: float = 1 - 1e-6, n: int = 400001):
    """r01 values at which the iteration's stopping step changes (a grid of n points, each transition bisected to double precision)"""
    g = np.linspace(lo, hi, n)
    _p, s = multiclass_p1(g)
    out = []
    for i in np.nonzero(s[1:] != s[:-1])[0]:
        a, b = g[i], g[i + 1]
        sa = multiclass_p1(np.array([a]))[1][0]
        for _ in range(60):
            m = 0.5 * (a + b)
            if multiclass_p1(np.array([m]))[1][0] == sa:
                a = m
            else:
                b = m
        out.append(0.5 * (a + b))
    return np.array(out)


# ---- seeded model draws ------------------------------------------------------------------------------------------------------

def random_svm(rng, nf: int, n_sv: int, gamma: float, balanced: bool = True) -> dict:
    """An SVM of nf features and n_sv support vectors for raw features about N(0, 1) per standardised unit: offsets N(0, 5), scales
    1 / U(0.5, 20), support vectors N(0, 1) in standardised units; dual coefficients of both signs, which with `balanced` sum to
    (nearly) zero as the SVM constraint makes them -- the decision then comes from cancellation, as the golden model's does."""
    coef = rng.standard_normal(n_sv) * rng.uniform(0.2, 3.0)
    if balanced and n_sv > 1:
        coef -= coef.mean()
    return {"offset": rng.normal(0.0, 5.0, nf).astype(F32), "scale": (1.0 / rng.uniform(0.5, 20.0, nf)).astype(F32),
            "sv": rng.standard_normal((n_sv, nf)).astype(F32), "coef": coef.astype(F32),
            "kernel_params": np.array([gamma, 0.0, 3.0], F32), "rho": np.array([rng.normal(0.0, 0.7)], F32),
            "prob_a": np.array([-rng.uniform(0.5, 3.0)], F32), "prob_b": np.array([rng.normal(0.0, 0.3)], F32),
            "vectors_per_class": np.array([n_sv - n_sv // 2, n_sv // 2], np.int64)}


def preimage(attrs: dict, z) -> np.ndarray:
    """raw float32 features whose Scaler output is (about) the standardised rows z: offset + z / scale"""
    off = np.asarray(attrs["offset"], np.float64)
    scl = np.asarray(attrs["scale"], np.float64)
    return (off + np.asarray(z, np.float64) / scl).astype(F32)


def probe_rows(rng, attrs: dict, n_each: int = 4) -> np.ndarray:
    """Feature rows at three distances from the support vectors: the preimages of SVs 0, 63, 64, 65 and the last (each lane-stride
    slot a bug could skip carries K ~ 1 on some row) and of a few random SVs, with and without a little noise; rows between SVs at
    gamma d2 ~ 0.1 .. 10; and rows so far out that every K underflows (gamma d2 > 150: dec == rho exactly).  gamma = 0 has no far
    rows (K = 1 everywhere)."""
    sv = np.asarray(attrs["sv"], np.float64)
    n_sv, nf = sv.shape
    gamma = float(F32(np.ravel(attrs["kernel_params"])[0]))
    picks = sorted({i for i in (0, 63, 64, 65, n_sv - 1) if i < n_sv} | set(rng.integers(0, n_sv, n_each).tolist()))
    z = [sv[picks], sv[picks] + 1e-3 * rng.standard_normal((len(picks), nf))]
    if gamma > 0:
        for t in (0.1, 1.0, 10.0):                                   # gamma d2 ~ t from a random SV
            base = sv[rng.integers(0, n_sv, n_each)]
            step = rng.standard_normal((n_each, nf))
            step *= math.sqrt(t / gamma) / np.linalg.norm(step, axis=1, keepdims=True)
            z.append(base + step)
        far = math.sqrt(150.0 / gamma) + float(np.abs(sv).max())
        z.append(rng.choice([-1.0, 1.0], (n_each, nf)) * far * rng.uniform(1.0, 1.5, (n_each, nf)))
    else:
        z.append(rng.standard_normal((3 * n_each, nf)) * 3.0)
    return preimage(attrs, np.concatenate(z))


def far_rows(attrs: dict, x) -> np.ndarray:
    """which rows x have every gamma d2_i > 150 (all K underflow in float32)"""
    ref = SvmRef(attrs)
    if ref.gamma == 0.0:
        return np.zeros(np.asarray(x).reshape(-1, ref.nf).shape[0], bool)
    z = ref.standardise(x).astype(np.float64)
    return np.array([float((((zr[None, :] - ref._sv64) ** 2).sum(axis=1)).min()) * ref.gamma > 150.0 for zr in z])


def svm_from_features(rng, feat, n_sv: int, gamma: float | None = None, noise: float = 0.3) -> dict:
    """An SVM fit to pooled features feat [N][nf] the way a trained one is: offset | scale = their mean | 1 / std (std 0 -> 1), SVs the
    standardised rows (cycled) plus N(0, noise) -- SV 0, 63, 64, 65 and the last exactly on a row, so that each lane-stride slot
    carries K ~ 1 on some clip -- and balanced dual coefficients; gamma default 1 / nf"""
    feat = np.asarray(feat, np.float64)
    n, nf = feat.shape
    mu, sd = feat.mean(axis=0), feat.std(axis=0)
    sd = np.where(sd > 0, sd, 1.0)
    attrs = random_svm(rng, nf, n_sv, 1.0 / nf if gamma is None else gamma)
    attrs["offset"], attrs["scale"] = mu.astype(F32), (1.0 / sd).astype(F32)
    z = SvmRef(attrs).standardise(feat.astype(F32)).astype(np.float64)
    sv = z[np.arange(n_sv) % n] + noise * rng.standard_normal((n_sv, nf))
    for k, i in enumerate(i for i in (0, 63, 64, 65, n_sv - 1) if i < n_sv):
        sv[i] = z[(7 * k + 3) % n]
    attrs["sv"] = sv.astype(F32)
    return attrs
