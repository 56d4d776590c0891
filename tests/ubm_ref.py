"""UBM training and the GMM quantiser (include/dsp_amd.h dsp_ubm_*, dsp_gmm_quantize) restated in numpy, from the formulas:

    model     log_const_k = log w_k - 0.5 sum_d log(2 pi var_kd),  c = mu,  ic = 1 / var
    per row   l_k = log_const_k - 0.5 sum_d (x_d - c_kd)^2 ic_kd,  m = max_k l_k, e_k = exp(l_k - m), S = sum e_k, p_k = e_k / S, ll = m + log S
    sums      N_k = sum_t p_k,  F_kd = sum_t p_k (x_d - c_kd),  G_kd = sum_t p_k (x_d - c_kd)^2,  L = sum_t ll
    M-step    N'_k = N_k + 10 eps, r_k = N_k / N'_k, delta = F / N', mean = r c + delta, E2 = G / N' + 2 c delta + r c^2,
              var = E2 - mean^2 + reg_covar,  w_k = N'_k / sum_j N'_j
    stop      lower_bound_i = L / n;  after iteration i when | lower_bound_i - lower_bound_(i-1) | < tol  (lower_bound_0 = -inf)
    start     means_i = row floor((i + 0.5) n / k), var = one k = 1 iteration from mean = row floor(n / 2), variance 1 (the global variance + reg_covar), w = 1 / k
    tables    means = rint(64 mean) -> int8, inv_covs = rint(2048 inv_cov) -> int32, log_consts = rint(256 log_const) -> int16, saturated

float64 by default.  dtype=np.float32 is the model of the GPU arithmetic: log_const, c and ic rounded once to float32 for the E-step, the
rows' terms and the sums inside a chunk of CHUNK_ROWS rows in float32 (ascending rows: strictly sequential), everything above the chunk
and the whole M-step in float64, L in float64.  numpy only; the posteriors are tests/enroll_ref.py's."""
import numpy as np

from tests import enroll_ref as E

CHUNK_ROWS = 256        # kUbmChunkRows of dsp_amd/csrc/ubm_kernels.hpp
GROUP_CHUNKS = 16       # kUbmGroupChunks
SUPER_GROUPS = 32       # kUbmSuperGroups
GATE_FACTOR = 8         # a GPU output may deviate from float64 by 8 x what this file's float32 model does on the same inputs
TINY = 10.0 * np.finfo(np.float64).eps


def log_consts(w, var):
    return np.log(np.asarray(w, np.float64)) - 0.5 * np.log(2.0 * np.pi * np.asarray(var, np.float64)).sum(axis=1)


def statistics(x, w, mu, var, dtype=np.float64):
    """-> (N [k], F [k][d], G [k][d], L, c [k][d]) in float64; c is what the moments are centred on (mu as the E-step has it)"""
    model = {"log_consts": log_consts(w, var).astype(dtype), "means": np.asarray(mu, np.float64).astype(dtype),
             "inv_covs": (1.0 / np.asarray(var, np.float64)).astype(dtype)}
    c = model["means"]
    k, d = c.shape
    N, F, G, L = np.zeros(k), np.zeros((k, d)), np.zeros((k, d)), 0.0
    x = np.asarray(x)
    for r0 in range(0, x.shape[0], CHUNK_ROWS):
        xc = x[r0:r0 + CHUNK_ROWS].astype(dtype)
        p, ll = E.posteriors(xc, model, dtype)
        dv = (xc[:, None, :] - c[None]).astype(dtype)
        pd = (p[:, :, None] * dv).astype(dtype)
        N += E._seq_sum(p, dtype).astype(np.float64)
        F += E._seq_sum(pd, dtype).astype(np.float64)
        G += E._seq_sum((pd * dv).astype(dtype), dtype).astype(np.float64)
        L += float(ll.astype(np.float64).sum())
    return N, F, G, L, c.astype(np.float64)


def m_step(N, F, G, c, reg_covar):
    """sklearn's _estimate_gaussian_parameters (diag) on moments centred on c -> (w, mu, var)"""
    n1 = N + TINY
    r = (N / n1)[:, None]
    delta = F / n1[:, None]
    mean = r * c + delta
    e2 = G / n1[:, None] + 2.0 * c * delta + r * c * c
    return n1 / n1.sum(), mean, e2 - mean * mean + reg_covar


def fit(x, init, max_iter=300, tol=1e-3, reg_covar=1e-6, dtype=np.float64, history=False):
    """EM from init = dict(weights, means, variances) -> dict(weights, means, variances, log_consts, inv_covs, lower_bounds [n_iter], n_iter,
    converged); history: also "models", the (w, mu, var) after every iteration"""
    w, mu, var = (np.asarray(init[key], np.float64) for key in ("weights", "means", "variances"))
    n = np.asarray(x).shape[0]
    bounds, models, prev, converged = [], [], -np.inf, False
    for _ in range(int(max_iter)):
        N, F, G, L, c = statistics(x, w, mu, var, dtype)
        w, mu, var = m_step(N, F, G, c, reg_covar)
        bounds.append(L / n)
        models.append((w, mu, var))
        if abs(bounds[-1] - prev) < tol:
            converged = True
            break
        prev = bounds[-1]
    out = result(w, mu, var)
    out.update(lower_bounds=np.array(bounds), n_iter=len(bounds), converged=converged)
    if history:
        out["models"] = models
    return out


def result(w, mu, var):
    return {"weights": w, "means": mu, "variances": var, "log_consts": log_consts(w, var), "inv_covs": 1.0 / var}


def init_row_indices(n, k):
    return np.array([((2 * i + 1) * int(n)) // (2 * int(k)) for i in range(int(k))], np.int64)


def init_rows(x, k, reg_covar=1e-6, dtype=np.float64):
    """the library's deterministic start -> dict(weights [k], means [k][d], variances [k][d])"""
    x = np.asarray(x)
    d = x.shape[1]
    N, F, G, _, c = statistics(x, np.ones(1), x[x.shape[0] // 2][None].astype(np.float64), np.ones((1, d)), dtype)
    var = m_step(N, F, G, c, reg_covar)[2][0]
    return {"weights": np.full(k, 1.0 / k), "means": x[init_row_indices(x.shape[0], k)].astype(np.float64), "variances": np.tile(var, (k, 1))}


def quantize(float_params):
    """-> (dict(means int8, inv_covs int32, log_consts int16), dict of the entries clamped per table); ties to even"""
    out, sat = {}, {}
    for key, scale, t in (("means", 64.0, np.int8), ("inv_covs", 2048.0, np.int32), ("log_consts", 256.0, np.int16)):
        q = np.rint(np.asarray(float_params[key], np.float64) * scale)
        lo, hi = float(np.iinfo(t).min), float(np.iinfo(t).max)
        sat[key] = int(((q < lo) | (q > hi)).sum())
        out[key] = np.clip(q, lo, hi).astype(t)
    return out, sat


def deviations(a, b):
    """max | a - b | of weights, means, log_consts and lower_bounds, max relative | a - b | / b of variances, between two fit results"""
    dev = {key: float(np.abs(np.asarray(a[key], np.float64) - np.asarray(b[key], np.float64)).max()) for key in ("weights", "means", "log_consts", "lower_bounds")}
    dev["variances"] = float((np.abs(np.asarray(a["variances"], np.float64) - b["variances"]) / b["variances"]).max())
    return dev


def gates(model32, want64):
    """per output GATE_FACTOR x the float32 model's deviation from float64, floored at 8 * 2^-23 * max | value | (1 for the relative one)"""
    dev = deviations(model32, want64)
    floor = {key: 8.0 * 2.0 ** -23 * float(np.abs(want64[key]).max()) for key in ("weights", "means", "log_consts", "lower_bounds")}
    floor["variances"] = 8.0 * 2.0 ** -23
    return {key: max(GATE_FACTOR * dev[key], floor[key]) for key in dev}


def draw_population(rng, ubm, n_rows):
    """rows of a population: components by the UBM's weights (never one at the 1e-6 variance floor), no speaker shift -> float32 [n][d]"""
    return E.draw_speaker(rng, ubm, n_rows, 0.0)
