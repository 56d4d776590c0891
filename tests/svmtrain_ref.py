"""Plain numpy float64 restatement of what dsp_svm_train_* computes, no GPU and no library: the Scaler fit, the distance matrix, libsvm's
SMO `Solver` (svm.cpp, without shrinking and with the library's tie rule), `sigmoid_train` and the fold rule of dsp_svm_folds.
tests/test_svmtrain_cpu.py pins it against sklearn's libsvm; tests/test_gpu_svmtrain.py holds the kernels to it.

Conventions (include/dsp_amd.h, SVM TRAINING): labels are 0 / 1 and label 0 is libsvm's positive side, y = +1; a problem is a list of
member rows (ascending), a box bound per label and gamma; K = exp(-gamma D2), dec = sum_i coef_i K_i + rho with coef_i = alpha_i y_i and
rho = -(libsvm's rho).  Where libsvm keeps the later of two tied candidates (`>=`, `<=`), the rule here keeps the lowest member index.
libsvm also rounds the rows of Q it caches to float32; here they stay float64 unless qfloat32 is asked for (dsp_svm_train_config.q_float32)."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
TAU = 1e-12
CONVERGED, MAX_ITER, ONE_CLASS, EMPTY = 0, 1, 2, 3
_MASK = (1 << 64) - 1


def scaler_fit(x, rows=None):
    """-> (offset, scale) float32: mean and 1 / population std (std 0 -> 1) of the float32 rows, in float64"""
    x = np.asarray(x, F32).astype(np.float64)
    if rows is not None:
        x = x[np.asarray(rows)]
    mean = x.mean(axis=0)
    std = np.sqrt(((x - mean) ** 2).mean(axis=0))
    return mean.astype(F32), np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 1.0).astype(F32)


def standardise(x, offset, scale):
    """the Scaler in float32: fl32(fl32(x - offset) * scale)"""
    x = np.asarray(x, F32)
    return ((x - np.asarray(offset, F32)).astype(F32) * np.asarray(scale, F32)).astype(F32)


def distances(z):
    """D2[n][n] float64 of float32 rows z, features added in ascending order"""
    z = np.asarray(z, F32).astype(np.float64)
    d2 = np.zeros((z.shape[0], z.shape[0]))
    for f in range(z.shape[1]):
        d = z[:, f][:, None] - z[:, f][None, :]
        d2 += d * d
    return d2


def _select(y, g, alpha, cb, krow_of):
    """-> (i, j, gap, K_i); i < 0: no candidate (gap -inf), j < 0: none with a positive gradient difference"""
    up = np.where(y > 0, alpha < cb, alpha > 0)
    if not up.any():
        return -1, -1, -math.inf, None
    v = np.where(up, -y * g, -np.inf)
    i = int(np.argmax(v))                                      # (argmax: the first of equals)
    gmax = v[i]
    ki = krow_of(i)
    low = np.where(y > 0, alpha > 0, alpha < cb)
    w = np.where(low, y * g, -np.inf)
    gmax2 = w.max()
    gd = gmax + w
    quad = 2.0 - 2.0 * ki
    quad = np.where(quad > 0, quad, TAU)
    with np.errstate(invalid="ignore"):
        obj = np.where(low & (gd > 0), -(gd * gd) / quad, np.inf)
    j = int(np.argmin(obj))
    return i, (j if np.isfinite(obj[j]) else -1), gmax + gmax2, ki


def _pair(yi, yj, gi, gj, ai, aj, ci, cj, kij):
    quad = 2.0 - 2.0 * kij
    if quad <= 0:
        quad = TAU
    if yi != yj:
        delta = (-gi - gj) / quad
        diff = ai - aj
        ai += delta
        aj += delta
        if diff > 0:
            if aj < 0:
                aj, ai = 0.0, diff
        elif ai < 0:
            ai, aj = 0.0, -diff
        if diff > ci - cj:
            if ai > ci:
                ai, aj = ci, ci - diff
        elif aj > cj:
            aj, ai = cj, cj + diff
    else:
        delta = (gi - gj) / quad
        s = ai + aj
        ai -= delta
        aj += delta
        if s > ci:
            if ai > ci:
                ai, aj = ci, s - ci
        elif aj < 0:
            aj, ai = 0.0, s
        if s > cj:
            if aj > cj:
                aj, ai = cj, s - cj
        elif ai < 0:
            ai, aj = 0.0, s
    return ai, aj


def solve(d2, labels, members, c0, c1, gamma, eps=1e-3, max_iter=10_000_000, qfloat32=False):
    """One problem on the shared matrix -> dict(status, coef float64 [n] (0 off the list), rho, n_iter, n_sv, n_bounded, objective, gap)"""
    n = d2.shape[0]
    members = np.asarray(members, np.int64)
    labels = np.asarray(labels)
    out = {"coef": np.zeros(n), "rho": 0.0, "n_iter": 0, "n_sv": 0, "n_bounded": 0, "objective": 0.0, "gap": 0.0, "const": 0.0}
    if members.size == 0:
        return dict(out, status=EMPTY)
    lab = labels[members]
    if (lab == 0).all() or (lab == 1).all():
        return dict(out, status=ONE_CLASS, const=1.0 if lab[0] == 0 else -1.0)
    y = np.where(lab == 0, 1.0, -1.0)
    cb = np.where(lab == 0, float(c0), float(c1))
    sub = d2[np.ix_(members, members)]
    alpha, g = np.zeros(members.size), -np.ones(members.size)

    def krow(t):
        k = np.exp(-gamma * sub[t])
        return k.astype(F32).astype(np.float64) if qfloat32 else k

    it, status = 0, CONVERGED
    while True:
        i, j, gap, ki = _select(y, g, alpha, cb, krow)
        if i < 0 or j < 0 or gap < eps:
            gap = 0.0 if i < 0 else gap
            break
        if it >= max_iter:
            status = MAX_ITER
            break
        kj = krow(j)
        ai, aj = _pair(y[i], y[j], g[i], g[j], alpha[i], alpha[j], cb[i], cb[j], ki[j])
        dai, daj = ai - alpha[i], aj - alpha[j]
        alpha[i], alpha[j] = ai, aj
        g += y * (y[i] * ki * dai + y[j] * kj * daj)
        it += 1
    upper, lower = alpha >= cb, alpha <= 0
    free = ~upper & ~lower
    yg = y * g
    if free.any():
        r = yg[free].sum() / free.sum()
    else:
        ub_set = (upper & (y < 0)) | (lower & ~upper & (y > 0))
        lb_set = (upper & (y > 0)) | (lower & ~upper & (y < 0))
        r = (yg[ub_set].min(initial=np.inf) + yg[lb_set].max(initial=-np.inf)) / 2
    out["coef"][members] = alpha * y
    return dict(out, status=status, rho=-r, n_iter=it, n_sv=int((alpha > 0).sum()), n_bounded=int(upper.sum()),
                objective=float((alpha * (g - 1.0)).sum() / 2), gap=float(gap))


def decisions(d2, sol, gamma):
    """dec float64 [n] of a solve() result for every row: members the training decision, the others the held-out one"""
    if sol["status"] in (ONE_CLASS, EMPTY):
        return np.full(d2.shape[0], sol["const"])
    sv = np.nonzero(sol["coef"])[0]
    return np.exp(-gamma * d2[:, sv]) @ sol["coef"][sv] + sol["rho"]


def violation_gap(d2, labels, members, coef, c0, c1, gamma, qfloat32=False):
    """the maximal violation m(alpha) - M(alpha) of the alphas behind `coef`, gradient recomputed from scratch (qfloat32: under the kernel
    rounded to float32, the problem libsvm and the trainer's q_float32 mode solve)"""
    members = np.asarray(members, np.int64)
    lab = np.asarray(labels)[members]
    y = np.where(lab == 0, 1.0, -1.0)
    cb = np.where(lab == 0, float(c0), float(c1))
    alpha = coef[members] * y
    k = np.exp(-gamma * d2[np.ix_(members, members)])
    g = y * ((k.astype(F32).astype(np.float64) if qfloat32 else k) @ coef[members]) - 1.0
    up = np.where(y > 0, alpha < cb, alpha > 0)
    low = np.where(y > 0, alpha > 0, alpha < cb)
    return float((-y * g)[up].max(initial=-np.inf) + (y * g)[low].max(initial=-np.inf))


def sigmoid_train(dec, labels):
    """libsvm's sigmoid_train on (dec, label) pairs, label 0 the positive class -> (A, B, n_iter)"""
    dec = np.asarray(dec, np.float64)
    pos = np.asarray(labels) == 0
    prior1, prior0 = float(pos.sum()), float((~pos).sum())
    t = np.where(pos, (prior1 + 1.0) / (prior1 + 2.0), 1.0 / (prior0 + 2.0))

    def fval(a, b):
        f = dec * a + b
        return float(np.where(f >= 0, t * f + np.log(1 + np.exp(-np.abs(f))), (t - 1) * f + np.log(1 + np.exp(-np.abs(f)))).sum())

    a, b = 0.0, math.log((prior0 + 1.0) / (prior1 + 1.0))
    fv = fval(a, b)
    it = 0
    for it in range(100):
        f = dec * a + b
        e = np.exp(-np.abs(f))
        p = np.where(f >= 0, e / (1 + e), 1 / (1 + e))
        q = np.where(f >= 0, 1 / (1 + e), e / (1 + e))
        d2, d1 = p * q, t - p
        h11, h22, h21 = 1e-12 + (dec * dec * d2).sum(), 1e-12 + d2.sum(), (dec * d2).sum()
        g1, g2 = (dec * d1).sum(), d1.sum()
        if abs(g1) < 1e-5 and abs(g2) < 1e-5:
            break
        det = h11 * h22 - h21 * h21
        da, db = -(h22 * g1 - h21 * g2) / det, -(-h21 * g1 + h11 * g2) / det
        gd = g1 * da + g2 * db
        step = 1.0
        while step >= 1e-10:
            na, nb = a + step * da, b + step * db
            nf = fval(na, nb)
            if nf < fv + 0.0001 * step * gd:
                a, b, fv = na, nb, nf
                break
            step /= 2
        if step < 1e-10:
            break
    else:
        it = 100
    return a, b, it


def mix(z: int) -> int:
    """splitmix64's finaliser, the library's 64-bit mix"""
    z &= _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def folds(n: int, k: int, seed: int) -> np.ndarray:
    """dsp_svm_folds: libsvm's shuffle (swap i with i + draw % (n - i)) on draws mix(seed + (i + 1) golden), fold f = perm[f n / k .. (f + 1) n / k)"""
    perm = list(range(n))
    for i in range(n):
        j = i + mix(seed + (i + 1) * 0x9E3779B97F4A7C15) % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    ids = np.empty(n, np.int32)
    for f in range(k):
        ids[perm[f * n // k:(f + 1) * n // k]] = f
    return ids


def balanced_weights(labels, c: float, rows=None):
    """sklearn's class_weight="balanced": C n / (2 n_class) per label -> (C0, C1)"""
    lab = np.asarray(labels)
    if rows is not None:
        lab = lab[np.asarray(rows)]
    n = lab.size
    return c * n / (2.0 * (lab == 0).sum()), c * n / (2.0 * (lab == 1).sum())


def fit(x, labels, c=10.0, gamma=None, fold_ids=None, k_prob=5, seed=0, eps=1e-3, max_iter=10_000_000, balanced=True):
    """dsp_svm_fit_device restated: Scaler on all rows, k_prob inner problems and the final one, the Platt fit on the held-out
    decisions, the compacted model -> (attrs dict for SvmModel / SvmRef, dict of the parts)"""
    x = np.asarray(x, F32)
    labels = np.asarray(labels, np.int32)
    n, nf = x.shape
    offset, scale = scaler_fit(x)
    z = standardise(x, offset, scale)
    if gamma is None:
        gamma = 1.0 / (nf * float(z.astype(np.float64).var()))
    d2 = distances(z)
    c0, c1 = balanced_weights(labels, c) if balanced else (c, c)
    ids = folds(n, k_prob, seed) if fold_ids is None else np.asarray(fold_ids, np.int32)
    rows = np.arange(n)
    dec_cv = np.empty(n)
    for f in range(k_prob):
        s = solve(d2, labels, rows[ids != f], c0, c1, gamma, eps, max_iter)
        dec_cv[ids == f] = decisions(d2, s, gamma)[ids == f]
    final = solve(d2, labels, rows, c0, c1, gamma, eps, max_iter)
    a, b, _ = sigmoid_train(dec_cv, labels)
    return model_from_training(z, labels, final["coef"], final["rho"], gamma, offset, scale, a, b), \
        {"final": final, "dec_cv": dec_cv, "fold_ids": ids, "d2": d2, "z": z, "gamma": gamma, "C": (c0, c1)}


def model_from_training(z, labels, coef, rho, gamma, offset, scale, prob_a, prob_b) -> dict:
    """the attrs dict of SvmModel: support vectors (rows with coef != 0) in libsvm's order, label 0's first"""
    labels = np.asarray(labels)
    sv = np.concatenate([np.nonzero((coef != 0) & (labels == k))[0] for k in (0, 1)])
    return {"offset": np.asarray(offset, F32), "scale": np.asarray(scale, F32), "sv": np.asarray(z, F32)[sv], "coef": coef[sv].astype(F32),
            "kernel_params": np.array([gamma, 0.0, 3.0], F32), "rho": np.array([rho], F32), "prob_a": np.array([prob_a], F32),
            "prob_b": np.array([prob_b], F32), "vectors_per_class": np.array([(labels[sv] == 0).sum(), (labels[sv] == 1).sum()], np.int64)}


# ---- the problems of tests/test_gpu_svmtrain.py ---------------------------------------------------------------------------------

def suite_problems(labels, c, gamma, nf):
    """The problems the GPU tests solve on one golden set, as (name, rows, C_label0, C_label1, gamma): all rows (sklearn's problem);
    one member per label; 63 / 64 / 65 members (across a wavefront) and 255 / 257 (across the block); one label with a single member;
    a box so small that every alpha is bounded (as many members of each label: rho comes from the midpoint of the bounds) and one so
    large that none is (16 members under gamma 50, a kernel close to the identity); gamma 0, 1 / nf and 50."""
    labels = np.asarray(labels)
    n = labels.size
    rows = np.arange(n, dtype=np.int32)
    r0, r1 = rows[labels == 0], rows[labels == 1]
    c0, c1 = float(c[0]), float(c[1])
    out = [("all", rows, c0, c1, gamma), ("two", np.sort(np.array([r0[0], r1[0]], np.int32)), c0, c1, gamma)]
    out += [(f"first{m}", rows[:m], c0, c1, gamma) for m in (63, 64, 65, 255, 257) if m <= n]
    out.append(("single", np.sort(np.concatenate([r1[:1], r0[:40]])), c0, c1, gamma))
    out.append(("bounded", np.sort(np.concatenate([r0[:30], r1[:30]])), 1e-3, 1e-3, gamma))
    out.append(("unbounded", rows[:16], 1e4, 1e4, 50.0))
    out += [("gamma0", rows[:65], 1.0, 1.0, 0.0), ("gamma1nf", rows[:65], 1.0, 1.0, 1.0 / nf), ("gamma50", rows[:65], 1.0, 1.0, 50.0)]
    return out


# max over a golden set's suite_problems of |dec_ref(1e-7) - dec_ref(1e-10)| over all rows, and of the same for rho, as
# tests/test_svmtrain_cpu.py measures and asserts it: what tests/test_gpu_svmtrain.py takes four times of as its parity allowance.
# "cv": the same over the problems of cv_reference on nf3.
SPREAD = {"nf40": 5.3e-8, "nf3": 2.4e-7, "nf1": 2.1e-7, "cepstrum": 6.9e-8, "cv": 2.0e-7}
# the same for the problem on all rows with the kernel rounded to float32 (solve(qfloat32=True)), the allowance of the q_float32 mode
SPREAD_Q32 = {"nf40": 5.1e-8, "nf3": 2.2e-7, "nf1": 9.9e-8, "cepstrum": 6.9e-8}
CV_GRID = ((1.0, 10.0), (0.1, "scale"))                       # Cs, gammas of the cross-validation tests
CV_FOLDS, CV_SEED = 3, 11


def cv_reference(x, labels, ids, cs, gammas, eps):
    """SvmTrainer.cross_validate restated: per outer fold the Scaler of the training rows, balanced box bounds of the training rows and
    every grid point solved on them -> held-out decisions float64 [grid][n]"""
    x = np.asarray(x, F32)
    labels = np.asarray(labels)
    n = labels.size
    held = np.zeros((len(cs) * len(gammas), n))
    for f in np.unique(ids):
        train, test = np.nonzero(ids != f)[0], np.nonzero(ids == f)[0]
        z = standardise(x, *scaler_fit(x, train))
        d2 = distances(z)
        scale_gamma = float(F32(1.0 / (x.shape[1] * z[train].astype(np.float64).var())))
        g = 0
        for c in cs:
            c0, c1 = balanced_weights(labels, c, train)
            for gamma in gammas:
                gamma = scale_gamma if gamma == "scale" else float(gamma)
                held[g, test] = decisions(d2, solve(d2, labels, train, c0, c1, gamma, eps), gamma)[test]
                g += 1
    return held
