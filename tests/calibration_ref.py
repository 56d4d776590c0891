"""The contract of score calibration (include/dsp_amd.h dsp_calibration_*) restated in numpy, float64 throughout: the
model c = A x + B + C l, the prior-weighted logistic objective with its gradient and Hessian, the damped Newton state machine with its
five end states, and apply.  The duration terms l are an INPUT here (log(n_frames + 1e-8) as the library's host code computes them:
ScoreCalibrator.duration_term), so that the library and the restatement start from the same numbers; duration_term below is np.log's."""
import numpy as np

CONVERGED, MAX_ITER, STALLED, SINGULAR, NO_CLASS = range(5)
MAX_HALVINGS = 30
REPORT_KEYS = ("a", "b", "c", "n_target", "n_nontarget", "n_excluded", "objective_start", "objective", "last_step", "n_iter", "n_rejected", "status")


def duration_term(n_frames):
    return np.log(np.asarray(n_frames, np.int64).astype(np.float64) + 1e-8)


def softplus(u):
    """log(1 + exp(u)) without overflow"""
    u = np.asarray(u, np.float64)
    return np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))


def sigmoid(u):
    u = np.asarray(u, np.float64)
    e = np.exp(-np.abs(u))
    return np.where(u >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _trials(scores, truth, duration):
    """-> (x, l, target) of the trials that take part, float64 / bool, and the number excluded"""
    x = np.asarray(scores, np.float32)
    x = x.reshape(x.shape[0], -1).astype(np.float64)
    T, S = x.shape
    truth = np.asarray(truth, np.int64)
    assert truth.shape == (T,)
    target = truth[:, None] == np.arange(S)[None, :]
    l = np.zeros(T) if duration is None else np.asarray(duration, np.float64)
    assert l.shape == (T,)
    l = np.broadcast_to(l[:, None], x.shape)
    keep = np.isfinite(x)
    return x[keep], l[keep], target[keep], int((~keep).sum())


def objective_parts(theta, x, l, target, prior, n_par):
    """J, g[n_par], H[n_par][n_par] at theta over the kept trials (both classes present)"""
    tau = np.log(prior / (1.0 - prior))
    a, b, c = theta
    z = a * x + b + c * l + tau
    P, N = int(target.sum()), int((~target).sum())
    w = np.where(target, prior / P, (1.0 - prior) / N)
    u = np.where(target, -z, z)
    J = float((w * softplus(u)).sum())
    s = sigmoid(u)
    dl = np.where(target, -s, s)
    phi = np.stack([x, np.ones_like(x), l][:n_par])
    g = (phi * (w * dl)).sum(axis=1)
    H = (phi[:, None, :] * phi[None, :, :] * (w * s * (1.0 - s))).sum(axis=2)
    return J, g, H


def cholesky_solve(H, g):
    """d with H d = g, or None: a pivot that is not above 0, or a d that is not finite"""
    n = g.size
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(i + 1):
                v = H[i, j] - float(L[i, :j] @ L[j, :j])
                if i == j:
                    if not v > 0.0:
                        return None
                    L[i, i] = np.sqrt(v)
                else:
                    L[i, j] = v / L[j, j]
        y = np.zeros(n)
        for i in range(n):
            y[i] = (g[i] - float(L[i, :i] @ y[:i])) / L[i, i]
        d = np.zeros(n)
        for i in range(n - 1, -1, -1):
            d[i] = (y[i] - float(L[i + 1:, i] @ d[i + 1:])) / L[i, i]
    return d if np.isfinite(d).all() else None


def newton_step(scores, truth, duration, theta, prior=0.5):
    """max |H^-1 g| at theta: what Newton would still move (inf where H cannot be factored)"""
    x, l, target, _ = _trials(scores, truth, duration)
    n_par = 2 if duration is None else 3
    _, g, H = objective_parts(theta, x, l, target, prior, n_par)
    d = cholesky_solve(H, g)
    return np.inf if d is None else float(np.abs(d).max())


def objective(scores, truth, duration, theta, prior=0.5):
    x, l, target, _ = _trials(scores, truth, duration)
    return objective_parts(theta, x, l, target, prior, 2 if duration is None else 3)[0]


def fit(scores, truth, duration=None, prior=0.5, tol=1e-10, max_iter=100, init=None, trace=None):
    """-> the report as a dict (REPORT_KEYS).  trace: a list that receives one (decision, J, J_base, max |theta - base|) per pass,
    decision "start" / "reject" / "accept" (J_base NaN and 0 at the start)"""
    x, l, target, n_excluded = _trials(scores, truth, duration)
    n_par = 2 if duration is None else 3
    init = np.array([1.0, 0.0, 0.0] if init is None else init, np.float64)
    P, N = int(target.sum()), int((~target).sum())
    rep = dict(n_target=P, n_nontarget=N, n_excluded=n_excluded, objective_start=np.nan, objective=np.nan, last_step=np.nan, n_iter=0, n_rejected=0)

    def end(status, theta, J):
        rep.update(a=float(theta[0]), b=float(theta[1]), c=float(theta[2]), objective=float(J), status=status)
        return rep

    if x.size + n_excluded == 0:
        return end(NO_CLASS, init, np.nan)
    if P == 0 or N == 0:
        rep["n_iter"] = 1
        return end(NO_CLASS, init, np.nan)
    theta, base, step = init.copy(), init.copy(), np.zeros(3)
    J_base, halvings, pending = np.nan, 0, False
    for it in range(max_iter):
        with np.errstate(all="ignore"):
            J, g, H = objective_parts(theta, x, l, target, prior, n_par)
        rep["n_iter"] = it + 1
        if it == 0:
            rep["objective_start"] = float(J)
        last = it == max_iter - 1
        if trace is not None:
            trace.append(("reject" if pending and not J <= J_base else "accept" if pending else "start", float(J), float(J_base),
                          float(np.abs(theta - base).max())))
        if pending and not J <= J_base:
            rep["n_rejected"] += 1
            halvings += 1
            if halvings > MAX_HALVINGS:
                return end(STALLED, base, J_base)
            theta = base - step * (1.0 / float(1 << halvings))
            if last:
                return end(MAX_ITER, base, J_base)
            continue
        if pending:
            moved = float(np.abs(theta - base)[:n_par].max())
            rep["last_step"] = moved
            if moved <= tol:
                return end(CONVERGED, theta, J)
        base, J_base, halvings = theta.copy(), J, 0
        d = cholesky_solve(H, g) if np.isfinite(J) and np.isfinite(g).all() and np.isfinite(H).all() else None
        if d is None:
            return end(SINGULAR, base, J)
        step = np.zeros(3)
        step[:n_par] = d
        theta = base - step
        pending = True
        if last:
            return end(MAX_ITER, base, J)
    raise AssertionError("unreachable")


def apply(scores, params, duration=None):
    """(float32)(A (double)x + B + C l), two or three roundings in float64 and one to float32; without duration terms the last term is
    left out"""
    x = np.asarray(scores, np.float32).astype(np.float64)
    a, b, c = (np.float64(v) for v in params)
    with np.errstate(all="ignore"):
        v = a * x + b
        if duration is not None:
            l = np.asarray(duration, np.float64)
            v = v + (c * l if x.ndim == 1 else (c * l)[:, None])
        return v.astype(np.float32)
