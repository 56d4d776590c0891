"""Float speaker verification (include/dsp_amd.h dsp_speaker_verif*) restated in numpy, from the formulas:

    model     the UBM's log_consts lc [k], means mu [k][d], inv_covs ic [k][d]; speaker s is (lc, means[s], ic) -- its own centres, the
              UBM's log_consts and inv_covs (mean-only MAP)
    per row   s = 0; ascending j: dv = x_j - c_kj, s = s + (dv dv) ic_kj;   l_k = lc_k - 0.5 s
              m = max_k l_k,  S = sum_k exp(l_k - m) over ascending k,  ll = m + log S
    per clip  L = sum_t (float64) ll_t: the clip's rows cut into tiles of TILE_ROWS from its first row; inside a tile the adjacent pairwise
              tree (1, 2, 4, .. 32 apart, absent rows 0); the tiles added in ascending order
    outputs   ll_ubm = L_u / n,  ll_target = L_s / n,  llr = (L_s - L_u) / n (the difference in float64),
              best = the smallest s with the largest llr,  best_llr = that value

float64 by default.  dtype=np.float32 is the model of the GPU arithmetic: the UBM rounded once to float32, every product and every
partial sum rounded to float32, S an ascending-k cumsum (strictly sequential), the row tree in float64 exactly as above, and each output
rounded once to float32.  numpy only."""
import numpy as np

TILE_ROWS = 64          # kVerifyTileRows of dsp_amd/csrc/verify_kernels.hpp
SPEAKER_TILE = 16       # kVerifySpeakerTile
GATE_FACTOR = 8         # a GPU output may deviate from float64 by 8 x what this file's float32 model does on the same inputs
OUTPUTS = ("llr", "ll_ubm", "ll_target", "best", "best_llr")


def row_ll(x, lc, c, ic, dtype=np.float64):
    """x [n][d] and one model (lc [k], c [k][d], ic [k][d]), all in `dtype` already -> ll [n] in `dtype`"""
    s = np.zeros((x.shape[0], lc.size), dtype)
    for j in range(x.shape[1]):                                                   # ascending d
        dv = (x[:, j:j + 1] - c[None, :, j]).astype(dtype)
        s = (s + ((dv * dv).astype(dtype) * ic[None, :, j]).astype(dtype)).astype(dtype)
    l = (lc[None] - (dtype(0.5) * s).astype(dtype)).astype(dtype)
    m = l.max(axis=1)
    e = np.exp((l - m[:, None]).astype(dtype)).astype(dtype)
    S = np.cumsum(e, axis=1, dtype=dtype)[:, -1]                                  # ascending k
    return (m + np.log(S).astype(dtype)).astype(dtype)


def clip_sum(ll):
    """ll [n] -> the float64 sum of the definition: tiles of TILE_ROWS, a pairwise tree inside each, the tiles in ascending order"""
    n = ll.shape[0]
    tiles = -(-n // TILE_ROWS)
    a = np.zeros(tiles * TILE_ROWS, np.float64)
    a[:n] = ll.astype(np.float64)
    a = a.reshape(tiles, TILE_ROWS)
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return float(np.cumsum(a[:, 0], dtype=np.float64)[-1])


def model_of(ubm, dtype=np.float64):
    """(lc, mu, ic) of the UBM dict, each float64 value rounded once to `dtype`"""
    return tuple(np.asarray(ubm[key], np.float64).astype(dtype) for key in ("log_consts", "means", "inv_covs"))


def clip_sums(x, ubm, means, dtype=np.float64):
    """one clip's rows x [n][d] -> (L_u, L [S]) in float64"""
    lc, mu, ic = model_of(ubm, dtype)
    x = np.asarray(x).astype(dtype)
    means = np.asarray(means).astype(dtype)
    return clip_sum(row_ll(x, lc, mu, ic, dtype)), np.array([clip_sum(row_ll(x, lc, c, ic, dtype)) for c in means], np.float64)


def verify(x, frame_offsets, ubm, means, dtype=np.float64):
    """clip c = rows [fo[c], fo[c + 1]) of x, means [S][k][d] -> dict(llr [C][S], ll_ubm [C], ll_target [C][S], best [C], best_llr [C]);
    float64 values by default, with dtype=np.float32 each rounded once to float32 as the library's are"""
    fo = np.asarray(frame_offsets, np.int64)
    n_clips, n_spk = fo.size - 1, np.asarray(means).shape[0]
    out = {"llr": np.zeros((n_clips, n_spk), dtype), "ll_ubm": np.zeros(n_clips, dtype), "ll_target": np.zeros((n_clips, n_spk), dtype),
           "best": np.zeros(n_clips, np.int32), "best_llr": np.zeros(n_clips, dtype)}
    for c in range(n_clips):
        n = int(fo[c + 1] - fo[c])
        if n < 1:
            raise ValueError(f"clip {c} has no rows")
        L_u, L = clip_sums(x[fo[c]:fo[c + 1]], ubm, means, dtype)
        out["ll_ubm"][c] = dtype(L_u / n)
        out["ll_target"][c] = (L / n).astype(dtype)
        out["llr"][c] = ((L - L_u) / n).astype(dtype)
        out["best"][c] = int(np.argmax(out["llr"][c]))                            # the first of the largest
        out["best_llr"][c] = out["llr"][c, out["best"][c]]
    return out


def gates(want, model):
    """per float output: GATE_FACTOR x | float32 model - float64 |, floored at GATE_FACTOR 2^-23 max | float64 value |"""
    g = {}
    for key in ("llr", "ll_ubm", "ll_target", "best_llr"):
        dev = float(np.abs(model[key].astype(np.float64) - want[key]).max())
        g[key] = max(GATE_FACTOR * dev, GATE_FACTOR * 2.0 ** -23 * float(np.abs(want[key]).max()))
    return g
