"""The seeded cases that tests/test_calibration_cpu.py (on the reference alone) and tests/test_gpu_calibration.py (against the library)
share, and the kernels' constants (dsp_amd/csrc/calibrate_kernels.hpp; the CPU test reads them out of the header and compares) from
which the shapes follow.

The statistics pass writes one partial per UNIT -- below LANES_ACROSS_COLUMNS columns a wavefront's ROWS_TIME rows of one column, from
there on a block's BLOCK_ROWS_COLUMNS rows of 64 columns -- and every further level of the tree adds FAN_IN partials, until FAN_IN or
fewer are left for the solve kernel.  tree(T, S) gives the nodes per level.

Scores are float32 normal variates, the targets' shifted up by 2: the classes overlap, the fit is well conditioned.  From 63 rows on
1 % of them are NaN, +inf and -inf, one of each at least.  truth is uniform over -1 .. S - 1 (at S = 1 a target in two of five rows), n_frames uniform over
50 .. 3000.  Everything is computed once per case and handed out read-only.

The seeds (SALT) are chosen on the reference alone so that every fit is DECISIVE.  The state machine accepts a pass when J <= J_base.  A
Newton step d lowers J by d'H d / 2: near 1e-16 of J for a step near 1e-8, which is the rounding noise of a float64 sum, so whether such
a pass is accepted is decided by rounding and may differ between two correct implementations.  Steps of 5e-7 and more move J by 3e-14
of itself and more on these cases, two orders above the noise: every implementation decides alike.  A fit is decisive at tol when no
full Newton step of it lies in (tol, 5e-7] (NOISE_ZONE).  Then the passes up to the first step of tol or less are the same everywhere; behind it come rejections by
rounding, any number of them, and one accepted pass that ends the fit.  So the status and the number of ACCEPTED passes, n_iter -
n_rejected, are the same everywhere, n_rejected is at least the reference's decisive rejections, and the parameters at the end lie
within the last full step, which is tol at most, of where it led: Newton's next step from there is tol at most.  n_iter and n_rejected
themselves are equal only where rounding decided alike."""
import functools

import numpy as np

from tests import calibration_ref as R

# dsp_amd/csrc/calibrate_kernels.hpp (LANES_ACROSS_COLUMNS: trial_kernels.hpp kTrialLanesAcrossColumns)
LANES_ACROSS_COLUMNS = 32
ROWS_TIME, ROWS_COLUMNS, BLOCK_ROWS_COLUMNS = 1024, 64, 256
FAN_IN = 16
SEED = 31119
TOL = 1e-8

# (T, S): the smallest matrices, both layouts with ragged ends, two shapes whose trees have two nodes or more at every level, and the
# reference's own shape
SHAPES = ((63, 1), (257, 3), (65, 32), (130, 70), (300000, 1), (5000, 70))
DEEP = ((300000, 1), (5000, 70))
SALT = {(63, 1): 4, (257, 3): 1, (65, 32): 2, (130, 70): 1, (300000, 1): 0, (5000, 70): 0}
NOISE_ZONE = 5e-7


def tree(T, S):
    """nodes per level: the units, then each reduction's, the last one FAN_IN or fewer"""
    n = -(-T // BLOCK_ROWS_COLUMNS) * -(-S // 64) if S >= LANES_ACROSS_COLUMNS else -(-T // ROWS_TIME) * S
    levels = [n]
    while n > FAN_IN:
        n = -(-n // FAN_IN)
        levels.append(n)
    return levels


def full_steps(trace):
    """the full Newton steps of a reference fit's trace: max |theta - base| of every pass that follows an accepted one"""
    return [trace[i][3] for i in range(1, len(trace)) if trace[i - 1][0] != "reject"]


def decisive(trace, tol=TOL):
    return all(not tol < step <= NOISE_ZONE for step in full_steps(trace))


def decisive_rejections(trace):
    """the rejections that rounding cannot have decided: J above J_base by more than 1e-13 of it (or not a number)"""
    return sum(1 for kind, J, J_base, _ in trace if kind == "reject" and not abs(J - J_base) <= 1e-13 * abs(J_base))


@functools.lru_cache(maxsize=None)
def case_inputs(T, S, salt=None):
    """-> (scores float32 [T][S], truth int32 [T], n_frames int64 [T]), read-only; salt None: the shape's own (SALT)"""
    salt = SALT.get((T, S), 0) if salt is None else salt
    rng = np.random.default_rng([SEED, T, S, salt])
    truth = np.where(rng.random(T) < 0.4, 0, -1) if S == 1 else rng.integers(-1, S, T)
    is_t = truth[:, None] == np.arange(S)[None, :]
    x = (rng.standard_normal((T, S)) + 2.0 * is_t).astype(np.float32)
    if T >= 63:
        u = rng.random((T, S))
        x[u < 0.004] = np.nan
        x[(u >= 0.004) & (u < 0.007)] = np.inf
        x[(u >= 0.007) & (u < 0.01)] = -np.inf
        x[5, 0], x[11, S - 1], x[17, 0] = np.nan, np.inf, -np.inf          # (the smallest hold one of each kind at least)
    n_frames = rng.integers(50, 3001, T).astype(np.int64)
    truth = truth.astype(np.int32)
    for a in (x, truth, n_frames):
        a.setflags(write=False)
    return x, truth, n_frames


def recorded(golden):
    """the reference's 92 recorded trials -> (scores float32 [92][1], truth, n_frames, the fixture)"""
    g = golden("gmm_calibration_ref.npz")
    return g["llr"].astype(np.float32).reshape(-1, 1), np.where(g["label"] == 1, 0, -1).astype(np.int32), g["n_frames"].astype(np.int64), g


def separable(T=92):
    """targets at 1 .. 1.1, non-targets at -1 .. -0.9: no finite optimum"""
    truth = np.where(np.arange(T) % 3 == 0, 0, -1).astype(np.int32)
    x = (np.where(truth == 0, 1.0, -1.0) + np.linspace(0.0, 0.1, T)).astype(np.float32).reshape(-1, 1)
    return x, truth


def saturated(T=200):
    """overlapping classes with |x| in 1 .. 2: from init A = -40 every |c| is 40 or more, sigma (1 - sigma) below 5e-18 and the Newton
    step beyond 1e16 -- still beyond 1e7 after 30 halvings, where the trials on the wrong side cost more than the start: DSP_CAL_STALLED"""
    rng = np.random.default_rng([SEED, T, 77])
    truth = np.where(rng.random(T) < 0.4, 0, -1).astype(np.int32)
    x = ((rng.random(T) + 1.0) * np.where(rng.random(T) < 0.85, 1, -1) * np.where(truth == 0, 1, -1)).astype(np.float32).reshape(-1, 1)
    return x, truth, (-40.0, 0.0, 0.0)


def duration(n_frames):
    """the duration terms as the library's host code computes them (no GPU needed): what the reference is fed"""
    import dsp_amd
    return dsp_amd.ScoreCalibrator.duration_term(n_frames)


@functools.lru_cache(maxsize=None)
def case_ref(T, S, with_frames):
    """the reference's fit of case_inputs(T, S) at TOL, from (1, 0, 0) -> (report, trace)"""
    x, truth, n_frames = case_inputs(T, S)
    trace = []
    return R.fit(x, truth, duration(n_frames) if with_frames else None, tol=TOL, trace=trace), tuple(trace)
