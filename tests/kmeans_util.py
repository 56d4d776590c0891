"""What tests/test_kmeans_cpu.py and tests/test_gpu_kmeans.py share: the cases of tests/golden/kmeans_ref.npz with the rows the library
is given, and the restatement's runs on them (computed once per session)."""
import numpy as np

from tests import kmeans_ref as K

CASES = ("strict", "strict32", "tol")
_cache = {}


def fixture(golden, tag):
    """(the npz, the float32 rows, sklearn's answers of the case as a dict)"""
    if tag not in _cache:
        z = golden("kmeans_ref.npz")
        x = z[f"{tag}__rows_q"].astype(np.float32) / np.float32(4096.0)
        sk = {key[len(tag) + 2:]: z[key] for key in z.files if key.startswith(tag + "__")}
        _cache[tag] = (z, x, sk)
    return _cache[tag]


def fixture_lloyd(golden, tag, dtype=np.float64):
    """tests/kmeans_ref.py's Lloyd on the case from its start, with the trace of every iteration"""
    if (tag, dtype) not in _cache:
        z, x, sk = fixture(golden, tag)
        _cache[(tag, dtype)] = K.lloyd(x, x.astype(np.float64)[sk["start"]], 300, float(z["tol"]), float(z["reg_covar"]), dtype, history=True)
    return _cache[(tag, dtype)]
