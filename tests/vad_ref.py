"""Voice activity detection (include/dsp_amd.h dsp_vad_*, dsp_rows_*) restated in float64 numpy, from its definition:
frame power over the sub-block tree, reference level, threshold, raw flags, Kaldi's smoothing, the hangover, the clips' records and
the selection.  Every sum is taken in the order the header states, so the device is held to these numbers bit for bit."""
import math

import numpy as np

COMPLETE, STREAM, CENTER = 0, 1, 2
REF_ABSOLUTE, REF_MAX, REF_MEAN = 0, 1, 2
TILE = 256
CLIP_DTYPE = np.dtype([("reference", "<f8"), ("threshold", "<f8"), ("n_raw", "<i4"), ("n_kept", "<i4"), ("first_kept", "<i4"), ("last_kept", "<i4")])


def lead_of(frame_length, hop, framing):
    return {COMPLETE: 0, STREAM: frame_length - hop, CENTER: frame_length // 2}[framing]


def geometry(frame_length, hop, framing):
    """(g, m, lead, W): samples per sub-block, sub-blocks per frame, samples of frame 0 before the clip, partials per sub-block"""
    lead = lead_of(frame_length, hop, framing)
    g = math.gcd(hop, frame_length)
    if lead:
        g = math.gcd(g, lead)
    quads, w = -(-g // 4), 1
    while w < quads and w < 64:
        w *= 2
    return g, frame_length // g, lead, w


def frames_for(n, frame_length, hop, framing):
    """dsp_mfcc_frames_for without a cap"""
    if framing == CENTER:
        return 1 + n // hop if n > 0 else 0
    if framing == STREAM:
        return -(-n // hop) if n > 0 else 0
    return 1 + (n - frame_length) // hop if n >= frame_length else 0


def halve(v):
    """v[..., 2^k] -> v[..., 0] after p[l] += p[l + off], off = 2^(k - 1) ... 1"""
    v = np.array(v, np.float64)
    off = v.shape[-1] // 2
    while off >= 1:
        v = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def subblock_sums(x, g, w):
    """s[b], b < ceil(n / g): the float64 sum of squares of samples [b g, b g + g), zero-extended, over the tree g fixes"""
    x = np.asarray(x, np.float32)
    nb = -(-x.size // g)
    turns = -(-(-(-g // 4)) // w)                      # quads per partial
    sq = np.zeros((nb, turns * w * 4), np.float64)
    padded = np.zeros(nb * g, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        padded[:x.size] = x.astype(np.float64) ** 2
        sq[:, :g] = padded.reshape(nb, g)
        sq = sq.reshape(nb, turns, w, 4)
        part = np.zeros((nb, w), np.float64)
        for turn in range(turns):
            for e in range(4):
                part = part + sq[:, turn, :, e]
        return halve(part)


def frame_power(x, frame_length, hop, framing, rows=None):
    """P[t] of one clip, float64; rows: fewer than the clip's length gives (a max_frames cap)"""
    g, m, lead, w = geometry(frame_length, hop, framing)
    x = np.asarray(x, np.float32)
    T = frames_for(x.size, frame_length, hop, framing) if rows is None else rows
    s = subblock_sums(x, g, w)
    nb = s.size
    b0 = (np.arange(T, dtype=np.int64) * hop - lead) // g
    total = np.zeros(T, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(m):
            b = b0 + j
            inside = (b >= 0) & (b < nb)
            total = np.where(inside, total + s[np.clip(b, 0, max(nb - 1, 0))] if nb else total, total)
        return total / np.float64(frame_length)


def frame_power_plain(x, frame_length, hop, framing, rows=None):
    """the independent form: np.mean(frame ** 2) over zero-padded frames, float64"""
    lead = lead_of(frame_length, hop, framing)
    x = np.asarray(x, np.float32).astype(np.float64)
    T = frames_for(x.size, frame_length, hop, framing) if rows is None else rows
    padded = np.concatenate([np.zeros(lead), x, np.zeros(frame_length + hop)])
    return np.array([np.mean(padded[t * hop:t * hop + frame_length] ** 2) for t in range(T)], np.float64).reshape(T)


def reference_level(P, reference):
    fin = np.isfinite(P)
    if reference == REF_ABSOLUTE:
        return 1.0
    if not fin.any():
        return 0.0
    if reference == REF_MAX:
        return float(P[fin].max())
    tiles = -(-P.size // TILE)
    v = np.zeros(tiles * TILE, np.float64)
    v[:P.size] = np.where(fin, P, 0.0)
    with np.errstate(over="ignore"):
        sums = halve(v.reshape(tiles, TILE))
        total = np.float64(0.0)
        for s in sums:
            total = total + s
        return float(total / np.float64(fin.sum()))


def threshold_of(ref, ratio, floor):
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float64(ref) * np.float64(ratio)
    return float(s) if s >= floor else float(floor)


def window_counts(flags, half):
    """(set flags, rows) in [max(0, t - half), min(T - 1, t + half)] for every t"""
    T = flags.size
    t = np.arange(T)
    lo, hi = np.maximum(0, t - half), np.minimum(T - 1, t + half)
    cum = np.concatenate([[0], np.cumsum(flags.astype(np.int64))])
    return cum[hi + 1] - cum[lo], hi - lo + 1


def decide(P, reference=REF_MAX, ratio=1e-6, floor=0.0, context=0, proportion=0.6, pad=0):
    """one clip -> (flags uint8 [T], record, raw, level_db float32 [T])"""
    P = np.asarray(P, np.float64)
    ref = reference_level(P, reference)
    thr = threshold_of(ref, ratio, floor)
    raw = np.isfinite(P) & (P > thr)
    if P.size:
        num, den = window_counts(raw, context)
        sm = num.astype(np.float64) >= den.astype(np.float64) * np.float64(proportion)
        keep = window_counts(sm, pad)[0] > 0
    else:
        keep = raw
    where = np.flatnonzero(keep)
    rec = np.zeros((), CLIP_DTYPE)
    rec["reference"], rec["threshold"], rec["n_raw"], rec["n_kept"] = ref, thr, int(raw.sum()), int(keep.sum())
    rec["first_kept"], rec["last_kept"] = (int(where[0]), int(where[-1])) if where.size else (-1, -1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        level = (10.0 * np.log10(P / np.float64(thr))).astype(np.float32)
    return keep.astype(np.uint8), rec, raw, level


def smooth_loop(raw, context, proportion, pad):
    """the smoothing and the hangover as a plain loop per row"""
    T = len(raw)
    sm = []
    for t in range(T):
        lo, hi = max(0, t - context), min(T - 1, t + context)
        sm.append(float(sum(bool(raw[u]) for u in range(lo, hi + 1))) >= float(hi - lo + 1) * proportion)
    return np.array([any(sm[u] for u in range(max(0, t - pad), min(T - 1, t + pad) + 1)) for t in range(T)], bool).reshape(T)


def trim_spans(records, offsets, hop):
    """librosa's trim: (starts, lengths, clips that keep something)"""
    offsets = np.asarray(offsets, np.int64)
    n = np.diff(offsets)
    has = records["n_kept"] > 0
    a = np.where(has, np.minimum(n, records["first_kept"].astype(np.int64) * hop), 0)
    b = np.where(has, np.minimum(n, (records["last_kept"].astype(np.int64) + 1) * hop), 0)
    return offsets[:-1] + a, b - a, int(has.sum())
