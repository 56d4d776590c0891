"""What tests/test_verify_scan_cpu.py and tests/test_gpu_verify_scan.py share: the synthetic recordings of the float speaker scan and,
per (case, window, hop), the float64 reference and the float32 model (tests/verify_scan_ref.py), computed once per session and never
changed.  The per-row ll of a case are computed once and serve all its scan configurations."""
import numpy as np

from tests import enroll_ref as E
from tests import verify_scan_ref as VS
from tests.verify_util import SHIFT_SIGMA, _freeze, offsets

SCAN_LENS = [1, 63, 97, 98, 107, 108, 257, 700]
SCAN_LEAD = 3                                       # rows of no recording in front of the first
SCAN_SEGMENT = 120                                  # a recording changes its speaker every 120 rows
SCAN_SPEAKERS = [1, 3, 16, 17, 33]
SCAN_KD = [(1, 1), (1, 16), (5, 13), (32, 13), (64, 16)]
SCAN_OTHER_D = [2, 7, 12]                            # further d of the kernels' dispatch, at k = 5 and (98, 10)
# (window, hop): one tile plus a part; exactly one tile; one row over a tile with hop near window; a window across the 256-row chunk;
# single rows; hop larger than window, with rows in no window
SCAN_CONFIGS = [(98, 10), (64, 1), (65, 64), (257, 100), (1, 1), (30, 45)]
_cache = {}


def scan_case(k, d):
    """a random UBM, 33 speakers enrolled by the restatement (float32 means) from 300 rows each of a shifted draw, and eight recordings
    stitched from consecutive 120-row segments of successive speakers' held-out rows (segment g of the batch: speaker g mod 33), so that
    `best` changes inside a recording; 3 rows of no recording (77) in front"""
    if (k, d) not in _cache:
        rng = np.random.default_rng(9000 + 100 * k + d)
        ubm = E.random_ubm(rng, k, d)
        n_spk = SCAN_SPEAKERS[-1]
        floor = k == 1                                                            # (the only component is the one at the floor)
        draws = [E.draw_speaker(rng, ubm, 300 + 700, SHIFT_SIGMA, skip_floor=not floor) for _ in range(n_spk)]
        means = np.stack([E.enroll(x[:300], ubm)["means"] for x in draws]).astype(np.float32)
        parts, g = [np.full((SCAN_LEAD, d), 77.0, np.float32)], 0
        for n in SCAN_LENS:
            for at in range(0, n, SCAN_SEGMENT):
                take = min(SCAN_SEGMENT, n - at)
                used = SCAN_SEGMENT * (g // n_spk)
                parts.append(draws[g % n_spk][300 + used:300 + used + take])
                g += 1
        feats = np.concatenate(parts)
        fo = offsets(SCAN_LENS, SCAN_LEAD)
        assert feats.shape == (fo[-1], d) and feats.dtype == np.float32
        ll = {dtype: VS.rows_ll(feats[fo[0]:], ubm, means, dtype) for dtype in (np.float64, np.float32)}
        _cache[(k, d)] = _freeze({"ubm": ubm, "feats": feats, "fo": fo, "means": means, "ll64": ll[np.float64], "ll32": ll[np.float32]})
    return _cache[(k, d)]


def scan_ref(k, d, window, hop):
    """-> (want, model): the float64 reference and the float32 model of the case's scan against all 33 speakers (verify_util.subset
    gives those of its first S)"""
    key = (k, d, window, hop)
    if key not in _cache:
        case = scan_case(k, d)
        base = int(case["fo"][0])
        _cache[key] = (_freeze(VS.scan_from_ll(case["ll64"], base, case["fo"], window, hop)),
                       _freeze(VS.scan_from_ll(case["ll32"], base, case["fo"], window, hop, np.float32)))
    return _cache[key]
