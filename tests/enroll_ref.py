"""Sliding CMVN and MAP enrolment (include/dsp_amd.h dsp_cmvn_*, dsp_speaker_enroll*) restated in numpy, from the formulas:

    CMVN      half = window // 2; row t of a recording of n rows: s = max(0, t - half), e = min(n, t + half),
              mu = mean x[s:e],  sigma = sqrt(mean (x[s:e] - mu)^2),  y[t] = (x[t] - mu) / (sigma + 1e-8)        per coefficient
    per row   l_k = log_const_k - 0.5 sum_d (x_d - mu_kd)^2 inv_cov_kd   (ascending d)
              m = max_k l_k, e_k = exp(l_k - m), S = sum_k e_k, p_k = e_k / S, ll = m + log S
    speaker   N_k = sum_t p_k, F_kd = sum_t p_k x_d, N'_k = N_k + 1e-8, alpha_k = N'_k / (N'_k + r) or fixed_alpha,
              mean_kd = alpha_k F_kd / N'_k + (1 - alpha_k) mu_kd,  q6 = clip(rint(64 mean), -128, 127)

float64 by default.  dtype=np.float32 is the model of the GPU arithmetic: the UBM rounded once to float32, every product and every
partial sum rounded to float32, sums over rows in ascending row order (np.cumsum: strictly sequential) -- except the sum of the rows' ll,
which the kernels keep in float64.  numpy only."""
import numpy as np

CHUNK_ROWS = 256        # kEnrollChunkRows of dsp_amd/csrc/enroll_kernels.hpp
CMVN_TILE_ROWS = 64     # kCmvnTileRows
CMVN_MAX_WINDOW = 2048  # kCmvnMaxWindow
GATE_FACTOR = 8         # a GPU output may deviate from float64 by 8 x what this file's float32 model does on the same inputs


def _seq_sum(a, dtype):
    """sum over axis 0 in ascending order, every partial sum rounded to dtype"""
    return np.cumsum(a, axis=0, dtype=dtype)[-1]


def cmvn(x, window, dtype=np.float64):
    """x [n][d] (one recording) -> y [n][d] in `dtype` arithmetic"""
    x = np.asarray(x).astype(dtype)
    n = x.shape[0]
    half = int(window) // 2
    y = np.zeros_like(x)
    for t in range(n):
        s, e = max(0, t - half), min(n, t + half)
        seg = x[s:e]
        cnt = dtype(e - s)
        mu = (_seq_sum(seg, dtype) / cnt).astype(dtype)
        dv = (seg - mu).astype(dtype)
        sigma = np.sqrt((_seq_sum((dv * dv).astype(dtype), dtype) / cnt).astype(dtype)).astype(dtype)
        y[t] = ((x[t] - mu).astype(dtype) / (sigma + dtype(1e-8)).astype(dtype)).astype(dtype)
    return y


def cmvn_ragged(x, frame_offsets, window, dtype=np.float64):
    """recording r = rows [fo[r], fo[r + 1]); rows of no recording stay zero"""
    x = np.asarray(x)
    y = np.zeros(x.shape, dtype)
    fo = np.asarray(frame_offsets, np.int64)
    for r in range(fo.size - 1):
        if fo[r + 1] > fo[r]:
            y[fo[r]:fo[r + 1]] = cmvn(x[fo[r]:fo[r + 1]], window, dtype)
    return y


def posteriors(x, ubm, dtype=np.float64):
    """x [n][d], ubm = dict(log_consts [k], means [k][d], inv_covs [k][d]) -> (p [n][k], ll [n])"""
    lc, mu, ic = (np.asarray(ubm[key], np.float64).astype(dtype) for key in ("log_consts", "means", "inv_covs"))
    x = np.asarray(x).astype(dtype)
    s = np.zeros((x.shape[0], lc.size), dtype)
    for j in range(x.shape[1]):
        dv = (x[:, j:j + 1] - mu[None, :, j]).astype(dtype)
        s = (s + ((dv * dv).astype(dtype) * ic[None, :, j]).astype(dtype)).astype(dtype)
    l = (lc[None] - (dtype(0.5) * s).astype(dtype)).astype(dtype)
    m = l.max(axis=1)
    e = np.exp((l - m[:, None]).astype(dtype)).astype(dtype)
    S = e.sum(axis=1, dtype=dtype)
    return (e / S[:, None]).astype(dtype), (m + np.log(S).astype(dtype)).astype(dtype)


def q6(means):
    """-> (int8 Q6 means: rint(64 mean), ties to even, saturated; the number of entries clamped per leading index)"""
    q = np.rint(np.asarray(means, np.float64) * 64.0)
    sat = ((q < -128) | (q > 127)).reshape(q.shape[0], -1).sum(axis=1) if q.ndim == 3 else int(((q < -128) | (q > 127)).sum())
    return np.clip(q, -128, 127).astype(np.int8), sat


def enroll(x, ubm, mode="relevance", relevance_factor=16.0, fixed_alpha=0.7, dtype=np.float64):
    """one speaker's rows x [n][d] -> dict(means [k][d], means_q6 int8, counts [k], ll_mean, saturated)"""
    if mode not in ("relevance", "fixed_alpha"):
        raise ValueError("mode must be 'relevance' or 'fixed_alpha'")
    x = np.asarray(x).astype(dtype)
    if x.shape[0] < 1:
        raise ValueError("a speaker needs at least one row")
    p, ll = posteriors(x, ubm, dtype)
    mu = np.asarray(ubm["means"], np.float64).astype(dtype)
    N = _seq_sum(p, dtype)
    F = _seq_sum((p[:, :, None] * x[:, None, :]).astype(dtype), dtype)
    n1 = (N + dtype(1e-8)).astype(dtype)
    alpha = (n1 / (n1 + dtype(relevance_factor))).astype(dtype) if mode == "relevance" else np.full_like(n1, dtype(fixed_alpha))
    means = (alpha[:, None] * F / n1[:, None] + (dtype(1.0) - alpha)[:, None] * mu).astype(dtype)
    mq, sat = q6(means)
    return {"means": means, "means_q6": mq, "counts": N, "ll_mean": dtype(ll.astype(np.float64).sum() / x.shape[0]), "saturated": sat}


def enroll_ragged(x, frame_offsets, ubm, dtype=np.float64, **kw):
    """speaker s = rows [fo[s], fo[s + 1]) -> dict of arrays stacked over the speakers"""
    fo = np.asarray(frame_offsets, np.int64)
    per = [enroll(x[fo[s]:fo[s + 1]], ubm, dtype=dtype, **kw) for s in range(fo.size - 1)]
    return {key: np.stack([np.asarray(r[key]) for r in per]) for key in ("means", "means_q6", "counts", "ll_mean", "saturated")}


def tie_zone(means64, gate_means):
    """entries whose float64 Q6 value a deviation of gate_means can move to the neighbouring integer: | frac(64 mean) - 0.5 | < 64 gate"""
    v = 64.0 * np.asarray(means64, np.float64)
    return np.abs((v - np.floor(v)) - 0.5) < 64.0 * gate_means


def weights_of(ubm):
    """the mixture weights behind log_consts = log w - 0.5 sum log(2 pi var)"""
    var = 1.0 / np.asarray(ubm["inv_covs"], np.float64)
    return np.exp(np.asarray(ubm["log_consts"], np.float64) + 0.5 * np.log(2.0 * np.pi * var).sum(axis=1))


def random_ubm(rng, k, d):
    """a UBM of the shape the library accepts: variances log-uniform in [1e-6, 4] with one component at the 1e-6 floor (the reference's
    UBM has one), means in the CMVN'd features' range"""
    var = np.exp(rng.uniform(np.log(1e-6), np.log(4.0), (k, d)))
    var[rng.integers(k)] = 1e-6
    w = rng.dirichlet(np.ones(k))
    return {"log_consts": np.log(w) - 0.5 * np.log(2.0 * np.pi * var).sum(axis=1), "means": rng.normal(0.0, 0.8, (k, d)), "inv_covs": 1.0 / var}


def fixture_feats(z):
    """the fixture's speakers as the library gets them: the stored raw rows (int16 / 32) through CMVN at window 300 in float64, float32"""
    raw = z["raw_q"].astype(np.float64) / 32.0
    return cmvn_ragged(raw, z["frame_offsets"], 300).astype(np.float32)


def draw_speaker(rng, ubm, n_rows, shift_sigma=0.35, skip_floor=True):
    """rows of a synthetic speaker: components chosen by the UBM's weights (skip_floor: never one at the 1e-6 variance floor), drawn from
    the component's Gaussian, moved by a per-speaker shift ~ N(0, shift_sigma^2) per dimension -> float32 [n_rows][d]"""
    var = 1.0 / np.asarray(ubm["inv_covs"], np.float64)
    w = weights_of(ubm) * ((var.min(axis=1) > 1.001e-6) if skip_floor else 1.0)
    comp = rng.choice(w.size, size=n_rows, p=w / w.sum())
    shift = rng.normal(0.0, shift_sigma, var.shape[1])
    return (np.asarray(ubm["means"], np.float64)[comp] + np.sqrt(var[comp]) * rng.normal(size=(n_rows, var.shape[1])) + shift).astype(np.float32)
