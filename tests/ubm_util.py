"""What tests/test_ubm_cpu.py and tests/test_gpu_ubm.py share: the golden fixture with the rows the library is given, and the float64
restatement's fit on it (computed once per session)."""
import os

import numpy as np

from tests import ubm_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ("iter1", "iter10", "tol")
_cache = {}


def fixture(golden):
    """(tests/golden/ubm_train_ref.npz, the float32 rows [6000][13], the start its sklearn answers were made from)"""
    if "fx" not in _cache:
        z = golden("ubm_train_ref.npz")
        x = z["rows_q"].astype(np.float32) / np.float32(4096.0)
        _cache["fx"] = (z, x, {key: z[f"init_{key}"] for key in ("weights", "means", "variances")})
    return _cache["fx"]


def fixture_fit(golden, dtype=np.float64):
    """tests/ubm_ref.py's fit on the fixture to the tol = 1e-3 stop, with the model after every iteration"""
    if ("fit", dtype) not in _cache:
        z, x, init = fixture(golden)
        _cache[("fit", dtype)] = U.fit(x, init, max_iter=300, tol=1e-3, reg_covar=float(z["reg_covar"]), dtype=dtype, history=True)
    return _cache[("fit", dtype)]
