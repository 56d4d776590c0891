"""What tests/test_snorm_cpu.py and tests/test_gpu_snorm.py share: the seeded cohorts, each with the records of the restatement
(tests/snorm_ref.py) computed once per session and never changed, the special vectors, and the gate against the independent form."""
import numpy as np

from tests import snorm_ref as R

# reduced lengths: the tile (64) and chunk (4096) edges of the tree, two chunks and a leaf, and the first length past the
# LDS-resident vector form (32 768 values)
LENGTHS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 33000]
# vector counts: the narrow form (below 32 columns) and the edges of the 64-column tile
VECTORS = [1, 2, 63, 64, 65, 130]
MAX_VECTORS = max(VECTORS)
SENTINEL = 0x5a5a5a5a5a5a5a5a
_cache = {}


def top_ks(n):
    """0 (all), 1, 2, n - 1, n, n + 5 and 300, those inside 0 .. 2^22, once each"""
    return sorted({k for k in (0, 1, 2, n - 1, n, n + 5, 300) if k >= 0})


def cohort(n, vectors=MAX_VECTORS, seed=0):
    """[vectors][n] float32: normal(-0.3, 0.5), a fifth of every vector's entries copied from one of its values, so that ties sit on the
    threshold of many top_k.  Read-only."""
    key = ("cohort", n, vectors, seed)
    if key not in _cache:
        rng = np.random.default_rng(9000 + 17 * n + seed)
        x = rng.normal(-0.3, 0.5, (vectors, n)).astype(np.float32)
        for v in x:
            v[rng.random(n) < 0.2] = v[rng.integers(n)]
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def special(n, vectors=70, seed=1):
    """[vectors][n] float32 (n >= 5) whose first ten vectors are the edge cases, the rest cohort(): NaN, +inf and -inf among the values;
    -0 and +0 around the threshold; all NaN; all equal (sigma = 0); a plateau of ties wider than any top_k below n / 2; only
    non-finite values; one finite value; a vector of -0 alone; values of both signs near the float32 limits.  Read-only."""
    key = ("special", n, vectors, seed)
    if key not in _cache:
        assert n >= 5 and vectors >= 10
        rng = np.random.default_rng(77 + n)
        x = cohort(n, vectors, seed).copy()
        x[0, ::3] = np.nan
        x[0, 1::7] = np.inf
        x[0, 2::5] = -np.inf
        x[1] = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))
        x[1, 0], x[1, 1] = 1.5, -2.0
        x[2] = np.nan
        x[3] = np.float32(0.7312)
        x[4] = rng.normal(0, 1, n).astype(np.float32)
        x[4, rng.permutation(n)[:max(2, (2 * n) // 3)]] = np.float32(2.5)                 # the plateau lies above most of the rest
        x[5] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), n)
        x[6] = np.nan
        x[6, n // 2] = -1.25
        x[7] = np.float32(-0.0)
        x[8] = rng.choice(np.array([3.0e38, -3.0e38, 1e-45, -1e-45, 1.0], np.float32), n)
        x[9] = -np.abs(x[9])
        x[9, 0] = -np.inf
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def records(x, top_k, name):
    """the restatement's records of the vectors (rows) of x, computed once per (name, top_k)"""
    key = ("records", name, top_k)
    if key not in _cache:
        rec = R.stats(x, R.PER_ROW, top_k)
        rec.setflags(write=False)
        _cache[key] = rec
    return _cache[key]


def same_bits(got, want):
    """records got == want, bit for bit on all six fields (NaN included) -> the first field that differs, or None"""
    for name in R.STAT_DTYPE.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            return name
    return None


def scores(rows, cols, seed=0):
    """[rows][cols] float32 trial scores, normal(-0.2, 0.6) with one NaN, one +inf and one -inf where there is room.  Read-only."""
    key = ("scores", rows, cols, seed)
    if key not in _cache:
        rng = np.random.default_rng(500 + 31 * rows + cols + seed)
        x = rng.normal(-0.2, 0.6, (rows, cols)).astype(np.float32)
        if x.size >= 8:
            flat = x.reshape(-1)
            flat[rng.permutation(flat.size)[:3]] = [np.nan, np.inf, -np.inf]
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def independent_records(x, top_k):
    """the independent form's (mean, std, threshold, n_finite, n_selected, n_above) of the vectors (rows) of x, as arrays"""
    cols = list(zip(*[R.independent_stat(v, top_k) for v in x]))
    return (np.array(cols[0], np.float64), np.array(cols[1], np.float64), np.array(cols[2], np.float32), np.array(cols[3], np.int32),
            np.array(cols[4], np.int32), np.array(cols[5], np.int32))


def gate_misses(got, x, mode, row, col, std_floor):
    """outputs `got` (float32) against the independent form: |got - ind| <= 1 float32 ulp of ind + 2^-40 (|x| + |mean|) / sigma'.  The
    second term is derived, not measured: two float64 summation orders over <= 2^22 terms differ by about depth * 2^-53 relative to
    sum |v|, some 2^-48 here; 2^-40 leaves eight bits; one ulp covers the final rounding.  Where the independent output is not finite
    the outputs must be the same infinity, or both NaN.  -> the number of outputs outside the gate"""
    ind, slack = R.independent_apply(x, mode, row, col, std_floor)
    with np.errstate(over="ignore"):
        ind32 = ind.astype(np.float32)                      # (beyond float32: the same infinity is asked of `got`)
    finite = np.isfinite(ind32)
    with np.errstate(invalid="ignore"):
        tol = np.spacing(np.abs(ind32[finite])).astype(np.float64) + slack[finite]
        bad = int((np.abs(got[finite].astype(np.float64) - ind[finite]) > tol).sum())
    rest_got, rest_ind = got[~finite], ind32[~finite]
    return bad + int((~((rest_got == rest_ind) | (np.isnan(rest_got) & np.isnan(rest_ind)))).sum())
