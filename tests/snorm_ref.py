"""Cohort normalisation of speaker scores (include/dsp_amd.h dsp_cohort_stats_device, dsp_score_normalize_device)
restated in numpy float64, bit for bit: the ordered keys, the threshold of the K closest cohort members by selection on the keys, the
float64 sums over the tree that the cohort's length alone fixes (chunks of 4096 from index 0, the adjacent pairwise tree inside a
chunk, the chunks added in ascending order) and the apply.  The oracle of tests/test_snorm_cpu.py and tests/test_gpu_snorm.py."""
import numpy as np

CHUNK = 4096
MAX_LENGTH = 1 << 22
MAX_VECTORS = 1 << 30
PER_ROW, PER_COLUMN = 0, 1
NORM_Z, NORM_T, NORM_S = 0, 1, 2
MODES = {"z": NORM_Z, "t": NORM_T, "s": NORM_S}
STAT_DTYPE = np.dtype([("mean", "<f8"), ("std", "<f8"), ("threshold", "<f4"), ("n_finite", "<i4"), ("n_selected", "<i4"), ("n_above", "<i4")])


def keys(v):
    """an unsigned that grows with the float, -0 before +0 (trial_kernels.hip key_of)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def float_of(key):
    k = np.asarray(key, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def tree_sum(leaves):
    """float64 leaves[n] (n >= 1) -> their sum over the tree n fixes"""
    leaves = np.asarray(leaves, np.float64)
    chunks = -(-leaves.size // CHUNK)
    x = np.zeros(chunks * CHUNK, np.float64)
    x[:leaves.size] = leaves
    x = x.reshape(chunks, CHUNK)
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    total = x[0, 0]
    for c in x[1:, 0]:
        total = total + c
    return total


def stat(v, top_k=0):
    """one cohort vector v[n] (float32) -> its record, a numpy scalar of STAT_DTYPE"""
    v = np.ascontiguousarray(v, np.float32)
    assert v.ndim == 1 and 1 <= v.size <= MAX_LENGTH and 0 <= top_k <= MAX_LENGTH
    out = np.zeros((), STAT_DTYPE)
    fin = np.isfinite(v)
    nf = int(fin.sum())
    if nf == 0:
        out["mean"] = out["std"] = out["threshold"] = np.nan
        return out
    kp = nf if (top_k == 0 or top_k > nf) else int(top_k)
    k = keys(v)
    tk = np.sort(k[fin])[::-1][kp - 1]
    theta = float_of(tk)
    sel = fin & (k > tk)
    g = int(sel.sum())
    e = np.float64(kp - g)
    assert kp - g >= 1
    vd = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        A = tree_sum(np.where(sel, vd, 0.0))
        mean = (A + e * np.float64(theta)) / np.float64(kp)
        d = vd - mean
        Q = tree_sum(np.where(sel, d * d, 0.0))
        dt = np.float64(theta) - mean
        p = dt * dt
        std = np.sqrt((Q + e * p) / np.float64(kp))
    out["mean"], out["std"], out["threshold"], out["n_finite"], out["n_selected"], out["n_above"] = mean, std, theta, nf, kp, g
    return out


def stats(cohort, axis, top_k=0):
    """cohort[R][C] float32 -> records [R] over the rows (PER_ROW) or [C] over the columns (PER_COLUMN)"""
    cohort = np.asarray(cohort, np.float32)
    assert cohort.ndim == 2 and axis in (PER_ROW, PER_COLUMN)
    vectors = cohort if axis == PER_ROW else cohort.T
    return np.array([stat(v, top_k) for v in vectors], STAT_DTYPE).reshape(-1)


def _side(x, st, std_floor):
    floor = np.float64(std_floor)
    sigma = np.where(st["std"] > floor, st["std"], floor)
    return x, np.where(st["n_finite"] > 0, st["mean"].astype(np.float64), np.nan), sigma


def apply(scores, mode, row_stats=None, col_stats=None, std_floor=1e-6):
    """scores[T][S] float32 -> the normalised scores, float32: z per column, t per row, s = 0.5 (z + t), float64 rounded once"""
    x = np.asarray(scores, np.float32).astype(np.float64)
    assert x.ndim == 2 and mode in (NORM_Z, NORM_T, NORM_S) and np.isfinite(std_floor) and std_floor >= 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode != NORM_T:
            _, mean, sigma = _side(x, col_stats, std_floor)
            z = (x - mean[None, :]) / sigma[None, :]
        if mode != NORM_Z:
            _, mean, sigma = _side(x, row_stats, std_floor)
            t = (x - mean[:, None]) / sigma[:, None]
        out = z if mode == NORM_Z else t if mode == NORM_T else np.float64(0.5) * (z + t)
        return out.astype(np.float32)


def independent_stat(v, top_k=0):
    """the independent form: the K' largest finite values as float64, sorted, numpy's own mean and std -> (mean, std, threshold,
    n_finite, n_selected, n_above)"""
    v = np.asarray(v, np.float32)
    f = v[np.isfinite(v)]
    if f.size == 0:
        return np.nan, np.nan, np.float32(np.nan), 0, 0, 0
    kp = f.size if (top_k == 0 or top_k > f.size) else int(top_k)
    order = np.argsort(keys(f), kind="stable")
    w = f[order][-kp:]
    theta = w[0]
    wd = w.astype(np.float64)
    return wd.mean(), wd.std(), theta, int(f.size), kp, int((keys(f) > keys(np.array([theta]))[0]).sum())


def independent_apply(scores, mode, row=None, col=None, std_floor=1e-6):
    """apply from (mean, std) pairs of the independent form -> (float64 outputs before the rounding, the gate's second term
    2^-40 (|x| + |mean|) / sigma' summed over the sides the mode uses and halved for s)"""
    x = np.asarray(scores, np.float32).astype(np.float64)
    parts, slack = [], []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for use, pair, shape in ((mode != NORM_T, col, (1, -1)), (mode != NORM_Z, row, (-1, 1))):
            if not use:
                continue
            mean, std = (np.asarray(a, np.float64).reshape(shape) for a in pair)
            sigma = np.where(std > std_floor, std, np.float64(std_floor))
            parts.append((x - mean) / sigma)
            slack.append(2.0 ** -40 * (np.abs(x) + np.abs(mean)) / sigma)
        if mode == NORM_S:
            return 0.5 * (parts[0] + parts[1]), 0.5 * (slack[0] + slack[1])
        return parts[0], slack[0]
