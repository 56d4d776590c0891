"""The k-means start of UBM training (include/dsp_amd.h dsp_kmeans_*) restated in numpy, from the formulas:

    draws     mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^ z >> 31 (mod 2^64)
              u(seed, j, t) = (mix(seed + (8 j + t + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53;  seed_r = mix((seed ^ 0xD1B54A32D192ED03) + (r + 1) * 0x9E37...)
    seeding   T = 2 + floor(ln k) trials; row_0 = floor(u(seed, 0, 0) n); m_i = min over the chosen rows of |x_i - x_row|^2; step j: pot = sum m,
              trial t proposes the first row with m_i > 0 whose cumulative sum of m exceeds u(seed, j, t) pot (past the end: the last row with
              m_i > 0); the proposal with the smallest sum_i min(m_i, |x_i - x_cand|^2) wins, ties to the lowest t; pot = 0 early: TooFewDistinctRows
    Lloyd     c = centre (as the labelling has it), s_k = sum_d (x_d - c_kd)^2, label = argmin_k s_k (ties to the lowest k);
              N_k, F_kd = sum (x_d - c_kd), G_kd = sum (x_d - c_kd)^2 over the rows labelled k; centre' = c + F / N (N = 0: the centre stays);
              stop: no label changed ("strict", first), else sum (centre' - centre)^2 <= tol mean_d var_d(x) ("tol"), else max_iter
    start     one more labelling against the final centres; N, F, G of it through tests/ubm_ref.py's m_step: weights, means, variances + reg_covar

float64 by default.  dtype=np.float32 is the model of the GPU arithmetic: c rounded once, the rows' terms and the sums inside a chunk of
CHUNK_ROWS rows in float32 (ascending rows), everything above the chunk and every update in float64; in the seeding m_i in float32 and
its sums in float64.  numpy only."""
import math

import numpy as np

from tests import ubm_ref as U

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_TRIALS = 6


class TooFewDistinctRows(ValueError):
    pass


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, j, t):
    return (mix(int(seed) + (8 * j + t + 1) * GOLDEN) >> 11) * 2.0 ** -53


def restart_seed(seed, r):
    return mix((int(seed) ^ 0xD1B54A32D192ED03) + (r + 1) * GOLDEN)


def trials(k):
    return 2 + int(math.floor(math.log(k)))


def sq_dists(x, c, dtype=np.float64):
    """x [n][d], c [k][d] -> s [n][k], summed over ascending d in `dtype`"""
    x, c = np.asarray(x).astype(dtype), np.asarray(c, np.float64).astype(dtype)
    s = np.zeros((x.shape[0], c.shape[0]), dtype)
    for j in range(x.shape[1]):
        dv = (x[:, j, None] - c[None, :, j]).astype(dtype)
        s = (s + (dv * dv).astype(dtype)).astype(dtype)
    return s


def propose(m, target):
    """the first row with m > 0 whose cumulative sum (float64, ascending) exceeds target; past the end the last row with m > 0"""
    cum = np.cumsum(m.astype(np.float64))
    hit = np.flatnonzero((cum > target) & (m > 0))
    return int(hit[0]) if hit.size else int(np.flatnonzero(m > 0)[-1])


def seed_rows(x, k, seed, dtype=np.float64):
    """greedy k-means++ -> int64 rows [k] in the order chosen"""
    x = np.asarray(x)
    n, T = x.shape[0], trials(k)
    rows = [min(int(draw(seed, 0, 0) * n), n - 1)]
    m = sq_dists(x, x[rows[0]][None], dtype)[:, 0]
    for j in range(1, k):
        pot = float(m.astype(np.float64).sum())
        if not pot > 0.0:
            raise TooFewDistinctRows(f"{j} centres chosen, every row sits on one of them")
        best, best_pot, best_m = -1, np.inf, None
        for t in range(T):
            cand = propose(m, draw(seed, j, t) * pot)
            mt = np.minimum(m, sq_dists(x, x[cand][None], dtype)[:, 0])
            pt = float(mt.astype(np.float64).sum())
            if pt < best_pot:
                best, best_pot, best_m = cand, pt, mt
        rows.append(best)
        m = best_m
    return np.array(rows, np.int64)


def seeding_is_valid(x, rows, seed):
    """The check of a seeding made in other arithmetic (float32, another summation order), replayed in float64 with ITS earlier choices:
    row 0 is the draw's; at step j, per trial, the acceptable rows are those with m > 0 whose cumulative interval holds u pot within
    eps pot, eps = 4 (d + 3) 2^-24; the row is acceptable for some trial, and it is the winner of SOME choice of one acceptable row per
    trial: its new potential is <= (1 + eps) x the largest new potential among each trial's acceptable rows.  (Against the smallest over
    ALL acceptable rows the float64 restatement's own seeding fails, whenever a draw falls within eps of a boundary and the neighbour it
    lets in is the better row: no arithmetic proposes that neighbour.)  The rows are distinct.  -> None, or a sentence saying what failed"""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    k, T, eps = len(rows), trials(len(rows)), 4.0 * (d + 3) * 2.0 ** -24
    if len(set(int(r) for r in rows)) != k:
        return "the rows are not distinct"
    if int(rows[0]) != min(int(draw(seed, 0, 0) * n), n - 1):
        return "row 0 is not the draw's"
    m = ((x - x[rows[0]]) ** 2).sum(axis=1)
    for j in range(1, k):
        pot = float(m.sum())
        cum = np.cumsum(m)
        per_trial = []
        for t in range(T):
            target = draw(seed, j, t) * pot
            ok = (m > 0) & (cum > target - eps * pot) & (cum - m <= target + eps * pot)
            per_trial.append([int(i) for i in np.flatnonzero(ok)])
        row = int(rows[j])
        if not any(row in a for a in per_trial):
            return f"step {j}: row {row} is acceptable for no trial"
        after = lambda i: float(np.minimum(m, ((x - x[i]) ** 2).sum(axis=1)).sum())      # noqa: E731
        mine = after(row)
        for t, a in enumerate(per_trial):
            if a and mine > (1.0 + eps) * max(after(i) for i in a):
                return f"step {j}: row {row} leaves potential {mine}, every acceptable row of trial {t} less"
        m = np.minimum(m, ((x - x[row]) ** 2).sum(axis=1))
    return None


def labelled_statistics(x, c, labels, dtype=np.float64):
    """-> (N [k], F [k][d], G [k][d]) in float64 of the rows by label, centred on c (as the labelling has it)"""
    x = np.asarray(x)
    c = np.asarray(c, np.float64).astype(dtype)
    k, d = c.shape
    N, F, G = np.zeros(k), np.zeros((k, d)), np.zeros((k, d))
    for r0 in range(0, x.shape[0], U.CHUNK_ROWS):
        xc = x[r0:r0 + U.CHUNK_ROWS].astype(dtype)
        p = (labels[r0:r0 + U.CHUNK_ROWS, None] == np.arange(k)[None]).astype(dtype)
        dv = ((xc[:, None, :] - c[None]) * p[:, :, None]).astype(dtype)
        N += np.cumsum(p, axis=0, dtype=dtype)[-1].astype(np.float64)
        F += np.cumsum(dv, axis=0, dtype=dtype)[-1].astype(np.float64)
        G += np.cumsum((dv * dv).astype(dtype), axis=0, dtype=dtype)[-1].astype(np.float64)
    return N, F, G


def label_rows(x, c, dtype=np.float64):
    """-> (labels int32 [n], s [n][k]) against c rounded to dtype"""
    s = sq_dists(x, c, dtype)
    return np.argmin(s, axis=1).astype(np.int32), s


def inertia_of(s, labels, dtype=np.float64):
    best = s[np.arange(s.shape[0]), labels]
    return float(sum(float(np.cumsum(best[r0:r0 + U.CHUNK_ROWS], dtype=dtype)[-1]) for r0 in range(0, best.size, U.CHUNK_ROWS)))


def shift_limit(x, tol):
    return float(tol) * float(np.asarray(x, np.float64).var(axis=0).mean())


def gmm_start(x, c, labels, reg_covar=1e-6, dtype=np.float64):
    """sklearn's _initialize for init_params="kmeans": _estimate_gaussian_parameters of the one-hot labels -> dict(weights, means, variances, counts)"""
    N, F, G = labelled_statistics(x, c, labels, dtype)
    w, mu, var = U.m_step(N, F, G, np.asarray(c, np.float64).astype(dtype).astype(np.float64), reg_covar)
    return {"weights": w, "means": mu, "variances": var, "counts": N.astype(np.int64)}


def lloyd(x, centres0, max_iter=300, tol=1e-4, reg_covar=1e-6, dtype=np.float64, history=False):
    """-> dict(centres, labels, counts, inertia, n_iter, stop, n_empty, weights, means, variances); history: also "trace", per iteration
    (the centres the rows were labelled against, the labels, the distances s)"""
    x = np.asarray(x)
    centres = np.array(centres0, np.float64)
    limit = shift_limit(x, tol)
    prev, trace, stop = None, [], "max_iter"
    n_iter = 0
    for _ in range(int(max_iter)):
        labels, s = label_rows(x, centres, dtype)
        N, F, _ = labelled_statistics(x, centres, labels, dtype)
        c = centres.astype(dtype).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            new = np.where(N[:, None] > 0, c + F / N[:, None], centres)
        shift = float(((new - centres) ** 2).sum(axis=1).sum())
        if history:
            trace.append((centres.copy(), labels, s, shift))
        centres = new
        n_iter += 1
        if prev is not None and np.array_equal(labels, prev):
            stop = "strict"
            break
        prev = labels
        if shift <= limit:
            stop = "tol"
            break
    labels, s = label_rows(x, centres, dtype)
    out = gmm_start(x, centres, labels, reg_covar, dtype)
    out.update(centres=centres, labels=labels, inertia=inertia_of(s, labels, dtype), n_iter=n_iter, stop=stop, n_empty=int((out["counts"] == 0).sum()))
    if history:
        out["trace"] = trace
    return out


def margins(s):
    """the relative label margin (s_2nd - s_1st) / s_2nd per row (1 where there is one centre)"""
    if s.shape[1] < 2:
        return np.ones(s.shape[0])
    two = np.partition(s.astype(np.float64), 1, axis=1)[:, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)


def rounding_bound(d):
    """the rounding bound of a d-term float32 sum of squares"""
    return 2.0 * (d + 3) * 2.0 ** -24


def train_ubm(x, k, seed, n_init=1, kmeans_max_iter=300, kmeans_tol=1e-4, dtype=np.float64, **em):
    """section 3: per restart seed, Lloyd, EM (tests/ubm_ref.py fit); the largest last lower bound wins, ties to the first -> (fit, report)"""
    fits, report = [], []
    for r in range(int(n_init)):
        rows = seed_rows(x, k, restart_seed(seed, r), dtype)
        km = lloyd(x, np.asarray(x)[rows].astype(np.float64), kmeans_max_iter, kmeans_tol, em.get("reg_covar", 1e-6), dtype)
        fit = U.fit(x, km, dtype=dtype, **em)
        fits.append(fit)
        report.append({"rows": rows, "kmeans_n_iter": km["n_iter"], "kmeans_stop": km["stop"], "lower_bound": float(fit["lower_bounds"][-1])})
    winner = int(np.argmax([r["lower_bound"] for r in report]))
    return fits[winner], {"winner": winner, "restarts": report}
