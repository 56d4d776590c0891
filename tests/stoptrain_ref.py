"""A float64 numpy restatement of stop-net training as include/dsp_amd.h states it (dsp_stop_train_*), no GPU and no
library: the library's draws, the epoch order, the initial weights, the Scaler (in the kernel's own summation tree, so that its float32
results are the kernel's bits), and a run -- Keras's fit with Adam, dropout, binary cross-entropy and EarlyStopping -- vectorised over
the batch.  The layer-1 feature sum is numpy's own (a matmul) by default; feature_order="asc" / "desc" take it strictly ascending /
descending, whose difference is the spread the device's allowance is four times of.

tests/test_stoptrain_cpu.py pins the restatement (torch.autograd, Adam's first step, early stopping) and the C ABI's host helpers against
it; tests/test_gpu_stoptrain.py and tests/test_gpu_stoptrain_shapes.py hold the kernels to it on the cases of case(); DEFECTS are
mistakes planted into it, by which tests/test_stoptrain_shapes_cpu.py shows what the cases can see."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
U64 = np.uint64
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-7
CONVERGED_EARLY, MAX_EPOCHS, NO_VALIDATION, EMPTY = 0, 1, 2, 3
HYPER = {"learning_rate": 1e-3, "dropout": (0.3, 0.3, 0.2), "batch_size": 32, "epochs": 50, "patience": 10, "restore_best": True}
FLOOR = 1e-9                                     # the allowance's floor, relative (the Platt fit's bound in DESIGN.md 3.20)


# ---- random numbers ----------------------------------------------------------------------------------------------------------------------

def mix(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, stream: int, counter: int) -> int:
    return mix(mix(seed + (stream + 1) * G) + (counter + 1) * G)


def uniform(seed: int, stream: int, counter: int) -> float:
    return (draw(seed, stream, counter) >> 11) * 2.0 ** -53


def _mix_v(z):
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uniform_v(seed: int, stream: int, counters) -> np.ndarray:
    """uniform() of an array of counters"""
    base = U64(mix(seed + (stream + 1) * G))
    with np.errstate(over="ignore"):
        d = _mix_v(base + (np.asarray(counters, U64) + U64(1)) * U64(G))
    return (d >> U64(11)).astype(np.float64) * 2.0 ** -53


def order(n: int, seed: int, epoch: int) -> np.ndarray:
    """the epoch's permutation of 0 .. n - 1: a 4-round Feistel network on the smallest even number of bits (>= 2) covering n, cycle-walked"""
    key = draw(seed, 1, epoch)
    half = 1
    while (1 << (2 * half)) < n:
        half += 1
    mask = U64((1 << half) - 1)
    x = np.arange(n, dtype=U64)
    todo = np.ones(n, bool)
    with np.errstate(over="ignore"):
        while todo.any():
            v = x[todo]
            l, r = v >> U64(half), v & mask
            for k in range(4):
                f = _mix_v(U64((key + (k + 1) * G) & M64) + r) & mask
                l, r = r, l ^ f
            v = (l << U64(half)) | r
            x[todo] = v
            idx = np.nonzero(todo)[0]
            todo[idx[v < U64(n)]] = False
    return x.astype(np.int32)


# ---- the model shape ------------------------------------------------------------------------------------------------------------------

def layer_sizes(n_coef: int, max_frames: int, units):
    """[(fan_in, fan_out)] of the four layers"""
    fan, out = n_coef * max_frames, []
    for u in units:
        out.append((fan, int(u)))
        fan = int(u)
    return out


def param_count(n_coef: int, max_frames: int, units) -> int:
    return sum(i * o + o for i, o in layer_sizes(n_coef, max_frames, units))


def unpack(params, n_coef: int, max_frames: int, units):
    """flat parameters -> ([W (in, out)] * 4, [b] * 4), copies"""
    ws, bs, k = [], [], 0
    for i, o in layer_sizes(n_coef, max_frames, units):
        ws.append(np.array(params[k:k + i * o], np.float64).reshape(i, o))
        k += i * o
        bs.append(np.array(params[k:k + o], np.float64))
        k += o
    return ws, bs


def pack(ws, bs) -> np.ndarray:
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in zip(ws, bs)])


def init(n_coef: int, max_frames: int, units, seed: int) -> np.ndarray:
    """the initial weights, flat: Glorot-uniform kernels on stream 0 (counter = flat index), zero biases"""
    out, k = np.zeros(param_count(n_coef, max_frames, units)), 0
    for i, o in layer_sizes(n_coef, max_frames, units):
        limit = math.sqrt(6.0 / (i + o))
        out[k:k + i * o] = (2.0 * uniform_v(seed, 0, np.arange(k, k + i * o)) - 1.0) * limit
        k += i * o + o
    return out


def model_from_training(n_coef: int, max_frames: int, units, params, mean, scale) -> dict:
    """the dict consumer_ref.StopNet / StopModel take: float32 roundings of the flat float64 parameters"""
    ws, bs = unpack(params, n_coef, max_frames, units)
    m = {"n_coef": n_coef, "max_frames": max_frames, "scaler_mean": np.asarray(mean, F32), "scaler_scale": np.asarray(scale, F32)}
    for l in range(4):
        m[f"kernel{l}"], m[f"bias{l}"] = ws[l].astype(F32).reshape(-1), bs[l].astype(F32)
    return m


# ---- dataset -------------------------------------------------------------------------------------------------------------------------

def used_frames(frame_offsets, max_frames: int) -> int:
    return int(min(max_frames, np.diff(np.asarray(frame_offsets, np.int64)).max()))


def used_index(n_coef: int, max_frames: int, t_used: int) -> np.ndarray:
    """input c * max_frames + t of used feature c * t_used + t"""
    return (np.arange(n_coef)[:, None] * max_frames + np.arange(t_used)[None, :]).reshape(-1)


def features(mfcc, frame_offsets, n_coef: int, max_frames: int) -> np.ndarray:
    """the used features [n][n_coef * t_used] float32 of a ragged matrix: frames past a clip's end are 0 (stop_detector.c:36-50)"""
    fo = np.asarray(frame_offsets, np.int64)
    t_used = used_frames(fo, max_frames)
    x = np.zeros((fo.size - 1, n_coef, t_used), F32)
    for i in range(fo.size - 1):
        t = min(int(fo[i + 1] - fo[i]), t_used)
        x[i, :, :t] = np.asarray(mfcc[fo[i]:fo[i] + t], F32).T
    return x.reshape(fo.size - 1, -1)


def _tree_sum(x: np.ndarray) -> np.ndarray:
    """the scaler kernel's sum over rows: lane l of 256 takes rows l, l + 256, ... ascending, a 6-level xor butterfly per wavefront, the
    four wavefronts as (0 + 1) + (2 + 3)"""
    part = np.zeros((256, x.shape[1]))
    for k0 in range(0, x.shape[0], 256):
        blk = x[k0:k0 + 256]
        part[:blk.shape[0]] += blk
    lane = np.arange(256)
    for s in (32, 16, 8, 4, 2, 1):
        part = part + part[lane ^ s]
    return (part[0] + part[64]) + (part[128] + part[192])


def scaler_fit(x_used, n_coef: int, max_frames: int, rows=None):
    """-> (mean, scale) float32 [n_coef * max_frames]: mean and population std (std 0 -> 1) over `rows`, float64 in the kernel's tree;
    inputs past the used frames are 0 and 1"""
    x = np.asarray(x_used, F32).astype(np.float64)
    if rows is not None:
        x = x[np.asarray(rows)]
    n = x.shape[0]
    mean = _tree_sum(x) / n
    d = x - mean
    sd = np.sqrt(_tree_sum(d * d) / n)
    idx = used_index(n_coef, max_frames, x.shape[1] // n_coef)
    m, s = np.zeros(n_coef * max_frames, F32), np.ones(n_coef * max_frames, F32)
    m[idx], s[idx] = mean.astype(F32), np.where(sd > 0, sd, 1.0).astype(F32)
    return m, s


def standardise(x_used, mean, scale, n_coef: int, max_frames: int) -> np.ndarray:
    """the inference expression on the used features: fl32(fl32(x - mean) / (scale == 0 ? 1 : scale))"""
    x = np.asarray(x_used, F32)
    idx = used_index(n_coef, max_frames, x.shape[1] // n_coef)
    m, s = np.asarray(mean, F32)[idx], np.asarray(scale, F32)[idx]
    return ((x - m).astype(F32) / np.where(s == 0, F32(1.0), s).astype(F32)).astype(F32)


# ---- a run ---------------------------------------------------------------------------------------------------------------------------

def sigmoid(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_from_logit(a, y):
    return np.maximum(a, 0.0) - a * y + np.log1p(np.exp(-np.abs(a)))


def _layer1(zb, w1, feature_order):
    if feature_order == "numpy":
        return zb @ w1
    prods = zb.T[:, :, None] * w1[:, None, :]                    # [F][B][u1]: a sum over axis 0 adds the features one after another
    return np.add.reduce(prods if feature_order == "asc" else prods[::-1], axis=0)


def dropout_masks(seed: int, gstep: int, batch: int, units, rates):
    """per hidden layer the kept flags [batch][units[l]] of optimiser step gstep (None: rate 0, no draw): kept when u >= rate on stream 2,
    counter = ((gstep * 3 + layer) * 256 + slot) * 16 + unit"""
    out = []
    for l in range(3):
        if not rates[l] > 0.0:
            out.append(None)
            continue
        c = ((gstep * 3 + l) * 256 + np.arange(batch)[:, None]) * 16 + np.arange(units[l])[None, :]
        out.append(uniform_v(seed, 2, c) >= rates[l])
    return out


def padded_units(u1: int) -> int:
    """the layer-1 width the kernels are instantiated at (stoptrain_kernels.hip padded_units): units u1 .. padded - 1 are padding"""
    return 4 if u1 <= 4 else (8 if u1 <= 8 else 16)


# Planted mistakes of the kind the kernels' index arithmetic could hold (tests/test_stoptrain_shapes_cpu.py): each is the identity on
# cases A, B and C.
#   w3_stride    every forward pass reads layer 3's kernel as w3[i * u2 + o] of the flat parameters behind it (bias3, kernel4, bias4,
#                then zeros) in place of w3[i * u3 + o]: nothing where u2 == u3
#   chunk_row    the first row of every 256-row evaluation chunk but the first (validation, prob, the dead-unit pass) takes the logit
#                of the row in front of it: nothing below 257 rows
#   padded_down  layer 1's padded width rounded down to a power of two (at least 4), the kernel of the units from there on read as 0
#                in every forward pass: nothing where u1 is 4, 8 or 16
DEFECTS = ("w3_stride", "chunk_row", "padded_down")


def _defective(ws, bs, defect):
    """the weights a forward pass with the planted mistake reads"""
    if defect == "w3_stride":
        u2, u3 = ws[2].shape
        flat = np.concatenate([ws[2].reshape(-1), bs[2], ws[3].reshape(-1), bs[3], np.zeros(u2 * u2)])
        ws = ws[:2] + [flat[np.arange(u2)[:, None] * u2 + np.arange(u3)[None, :]]] + ws[3:]
    elif defect == "padded_down":
        u1 = ws[0].shape[1]
        wrong = max(4, 1 << (u1.bit_length() - 1))
        ws = [np.where(np.arange(u1)[None, :] < wrong, ws[0], 0.0)] + ws[1:]
    return ws


def forward(ws, bs, zb, masks=None, scales=(1.0, 1.0, 1.0), feature_order="numpy", defect=None):
    """-> (logits [B], [h1, h2, h3]): ReLU hidden layers, inverted dropout where masks are given"""
    hs, h = [], None
    if defect is not None:
        ws = _defective(ws, bs, defect)
    for l in range(3):
        a = (_layer1(zb, ws[0], feature_order) if l == 0 else h @ ws[l]) + bs[l]
        h = np.maximum(a, 0.0)
        if masks is not None and masks[l] is not None:
            h = np.where(masks[l], h * scales[l], 0.0)
        hs.append(h)
    return (h @ ws[3])[:, 0] + bs[3][0], hs


def batch_gradient(ws, bs, zb, yb, masks=None, scales=(1.0, 1.0, 1.0), feature_order="numpy", defect=None):
    """-> (per-sample losses [B], [gW] * 4, [gb] * 4) of the batch's mean loss"""
    a, hs = forward(ws, bs, zb, masks, scales, feature_order, defect)
    d = (sigmoid(a) - yb) / yb.size
    gw, gb = [None] * 4, [None] * 4
    gw[3], gb[3] = hs[2].T @ d[:, None], np.array([d.sum()])
    d = np.where(hs[2] > 0, (d[:, None] * ws[3][:, 0][None, :]) * scales[2], 0.0)
    for l in (2, 1):
        gw[l], gb[l] = hs[l - 1].T @ d, d.sum(axis=0)
        d = np.where(hs[l - 1] > 0, (d @ ws[l].T) * scales[l - 1], 0.0)
    gw[0], gb[0] = zb.T @ d, d.sum(axis=0)
    return bce_from_logit(a, yb), gw, gb


def adam_step(w, m, v, g, lr: float, t: int):
    """Keras's Adam in place, t = 1, 2, ..."""
    lr_t = lr * math.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
    m *= BETA1
    m += (1.0 - BETA1) * g
    v *= BETA2
    v += (1.0 - BETA2) * (g * g)
    w -= lr_t * m / (np.sqrt(v) + ADAM_EPS)


class EarlyStopping:
    """Keras's callback: val_loss < best (strict; NaN never improves) is an improvement, otherwise ++wait and wait >= patience stops"""

    def __init__(self, patience: int):
        self.patience, self.best, self.best_epoch, self.wait, self.margin = patience, math.inf, -1, 0, math.inf

    def update(self, val_loss: float, epoch: int):
        """-> (improved, stop)"""
        if not math.isnan(val_loss) and math.isfinite(self.best):
            self.margin = min(self.margin, abs(val_loss - self.best))
        if val_loss < self.best:
            self.best, self.best_epoch, self.wait = val_loss, epoch, 0
            return True, False
        self.wait += 1
        return False, self.wait >= self.patience


def early_stopping(val_losses, patience: int, epochs: int):
    """the callback over a given val_loss sequence -> (n_epochs, best_epoch, the epoch whose weights are restored or -1)"""
    es, n = EarlyStopping(patience), 0
    for e in range(epochs):
        n = e + 1
        if es.update(float(val_losses[e]), e)[1]:
            break
    return n, es.best_epoch, es.best_epoch


def evaluate(ws, bs, zb, feature_order="numpy", defect=None):
    """forward() without dropout over rows in the kernels' chunks of 256"""
    if defect == "chunk_row" and zb.shape[0] > 256:
        first = np.arange(256, zb.shape[0], 256)
        zb = zb.copy()
        zb[first] = zb[first - 1]
    return forward(ws, bs, zb, feature_order=feature_order, defect=defect)


def train_run(z, labels, n_coef: int, max_frames: int, units, run: dict, feature_order="numpy", defect=None):
    """One run on the standardised used features z [n][F_used] float32 -> dict(history [epochs][2], params flat [n_params], prob [n],
    n_epochs, best_epoch, best_val_loss, last_loss, status, val_correct, n_dead_units, margin: the smallest |val_loss - best| any
    early-stopping comparison saw, p_margin: the smallest |P - 0.5| over the validation rows).  defect: one of DEFECTS, planted."""
    h = {**HYPER, **run}
    z = np.asarray(z, F32).astype(np.float64)
    y_all = np.asarray(labels).astype(np.float64)
    train_rows = np.asarray(h["train_rows"], np.int64).reshape(-1)
    val_rows = np.asarray(h["val_rows"] if h.get("val_rows") is not None else [], np.int64).reshape(-1)
    seed, lr, rates, batch, epochs = int(h.get("seed", 0)), float(h["learning_rate"]), [float(r) for r in h["dropout"]], int(h["batch_size"]), int(h["epochs"])
    scales = [1.0 / (1.0 - r) for r in rates]
    idx = used_index(n_coef, max_frames, z.shape[1] // n_coef)
    full = init(n_coef, max_frames, units, seed)
    ws, bs = unpack(full, n_coef, max_frames, units)
    w1_full = ws[0]
    ws[0] = w1_full[idx].copy()
    state = ws + bs
    ms, vs = [np.zeros_like(p) for p in state], [np.zeros_like(p) for p in state]
    history = np.full((epochs, 2), np.nan)
    es = EarlyStopping(int(h["patience"]))
    best_state, n_epochs, last_loss, gstep = None, 0, math.nan, 0
    status = EMPTY if train_rows.size == 0 else (NO_VALIDATION if val_rows.size == 0 else MAX_EPOCHS)
    for epoch in range(epochs if train_rows.size else 0):
        perm = train_rows[order(train_rows.size, seed, epoch)]
        total = 0.0
        for s0 in range(0, perm.size, batch):
            rows = perm[s0:s0 + batch]
            masks = dropout_masks(seed, gstep, rows.size, units, rates)
            loss, gw, gb = batch_gradient(ws, bs, z[rows], y_all[rows], masks, scales, feature_order, defect)
            total += loss.sum() / rows.size * rows.size
            gstep += 1
            for p, m, v, g in zip(state, ms, vs, gw + gb):
                adam_step(p, m, v, g, lr, gstep)
        last_loss = total / train_rows.size
        n_epochs = epoch + 1
        val_loss = math.nan
        if val_rows.size:
            val_loss = float(bce_from_logit(evaluate(ws, bs, z[val_rows], feature_order, defect)[0], y_all[val_rows]).sum() / val_rows.size)
        history[epoch] = last_loss, val_loss
        if val_rows.size:
            improved, stop = es.update(val_loss, epoch)
            if improved:
                best_state = [p.copy() for p in state]
            if stop:
                status = CONVERGED_EARLY
                break
    if h["restore_best"] and val_rows.size and best_state is not None:
        state = best_state
    ws, bs = state[:4], state[4:]
    prob = sigmoid(evaluate(ws, bs, z, feature_order, defect)[0])
    dead = 0
    if train_rows.size:
        dead = int(sum((hl.max(axis=0) <= 0).sum() for hl in evaluate(ws, bs, z[train_rows], feature_order, defect)[1]))
    w1 = w1_full.copy()
    w1[idx] = ws[0]
    return {"history": history, "params": pack([w1] + ws[1:], bs), "prob": prob, "n_epochs": n_epochs, "best_epoch": es.best_epoch,
            "best_val_loss": es.best if es.best_epoch >= 0 else math.nan, "last_loss": last_loss, "status": status,
            "val_correct": int(((prob[val_rows] > 0.5) == (y_all[val_rows] == 1)).sum()), "n_dead_units": dead, "margin": es.margin,
            "p_margin": float(np.abs(prob[val_rows] - 0.5).min()) if val_rows.size else math.inf}


def relative(a, b) -> float:
    """the largest difference of two arrays relative to the larger array's largest magnitude (NaNs must coincide)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    if not ok.any():
        return 0.0
    return float(np.abs(a[ok] - b[ok]).max() / max(np.abs(a[ok]).max(), np.abs(b[ok]).max(), 1e-300))


# ---- the GPU tests' cases (tests/test_gpu_stoptrain*.py), shared with the spread test ------------------------------------------------------

def planted(seed: int, n_coef: int, lengths, frames_for_direction: int):
    """A seeded synthetic set with consumer_ref's data shape: ragged MFCC rows, and labels separable by a planted direction over the first
    frames -> (mfcc [F][n_coef] float32, frame_offsets int64, labels int32)"""
    from tests import consumer_ref as CR
    rng = np.random.default_rng(seed)
    shape = CR.stop_data_shape(rng, n_coef)
    fo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    mfcc = CR.stop_rows(rng, shape, int(fo[-1]))
    direction = rng.standard_normal((min(frames_for_direction, min(lengths)), n_coef)) / shape[1]
    labels = np.arange(len(lengths)) % 2
    for i in range(len(lengths)):                                  # push the first frames along the direction, by the label's sign
        k = direction.shape[0]
        mfcc[fo[i]:fo[i] + k] += ((2 * labels[i] - 1) * 1.5 * shape[1] * np.sign(direction)).astype(F32)
    return mfcc, fo, labels.astype(np.int32)


OFF = (0.0, 0.0, 0.0)
# name: n_coef, max_frames, units, clips, frames per clip (one number, or lo .. hi drawn with both ends present), n_train, the runs' base
SHAPES = {
    "A": (3, 7, (4, 2, 2, 1), 23, (2, 9), 17, dict(batch_size=4, epochs=6, patience=10, learning_rate=1e-2)),
    "B": (13, 50, (16, 16, 16, 1), 70, 50, 50, dict(batch_size=32, epochs=5, patience=10, learning_rate=1e-3)),
    "C": (13, 500, (4, 2, 2, 1), 40, 98, 30, dict(batch_size=32, epochs=12, patience=3, learning_rate=3e-2)),
    "D": (5, 9, (7, 3, 5, 1), 600, (3, 11), 300, dict(batch_size=256, epochs=6, patience=10, learning_rate=1e-2)),
    "E": (2, 6, (1, 1, 1, 1), 40, (2, 7), 25, dict(batch_size=4, epochs=6, patience=10, learning_rate=1e-2)),
    "F": (4, 70, (12, 16, 9, 1), 90, 70, 60, dict(batch_size=16, epochs=4, patience=10, learning_rate=1e-2)),
    "G": (16, 16, (3, 5, 2, 1), 50, 16, 33, dict(batch_size=8, epochs=5, patience=10, learning_rate=1e-2)),
    "H": (3, 11, (8, 16, 1, 1), 60, (2, 8), 40, dict(batch_size=8, epochs=5, patience=10, learning_rate=1e-2)),
}
CASES_OLD, CASES_NEW = ("A", "B", "C"), ("D", "E", "F", "G", "H")
ODD_BATCH = {"E": 3, "F": 7, "G": 5, "H": 3}       # no multiple of 32 / padded_units(u1), the samples layer 1 takes at a time
# Chosen on the CPU, from the restatement alone, so that every deciding val_loss comparison of the cases' runs has a margin above 1e-6, every
# validation row's |P - 0.5| too, and the ascending, descending and numpy-order restatements agree on every integer result
# (test_restatement_spread asserts it).  Measured, spread between the ascending and descending layer-1 sums / smallest margin / smallest
# p_margin over the case's runs:
#   A 6.1e-16   B 5.0e-15   C 6.5e-15   (margins in tests/test_stoptrain_cpu.py)
#   D 3.4e-15 / 6.1e-3 / 5.8e-4   (the patience-0 pair: 4 epochs, best epoch 2, margin 2.2e-2)
#   E 2.4e-16 / 3.7e-4 / 2.5e-3
#   F 2.0e-15 / 1.5e-3 / 1.9e-4
#   G 1.2e-15 / 1.5e-2 / 9.4e-4
#   H 4.9e-15 / 3.5e-3 / 2.9e-4
# so the allowance max(4 x spread, FLOOR) is FLOOR = 1e-9 in every case.
CASE_SEEDS = {"A": 100, "B": 100, "C": 110, "D": 100, "E": 100, "F": 100, "G": 100, "H": 100}
# case D's patience-0 pair: seed and learning rate at which the restatement's val_loss rises before the last epoch, so that the run stops
# early one epoch behind its best and restore_best decides which weights come back
D_STOP = dict(seed=201, learning_rate=1e-1)


def case(name: str) -> dict:
    """the cases of DESIGN.md 3.21: shapes, data and the runs the GPU tests train.  A, B, C: dropout on, off, batch 1, batch >= n_train.
    D: the row-count edges (300 training rows, 300 validation rows, batch 256 / 37 without restore_best / 33 / 1 and the patience-0
    pair with and without restore_best).  E .. H: dropout on, off, ODD_BATCH, batch >= n_train."""
    n_coef, max_frames, units, n, frames, n_train, base = SHAPES[name]
    rng = np.random.default_rng(11 + "ABCDEFGH".index(name))
    if isinstance(frames, tuple):
        lengths = [int(v) for v in rng.integers(frames[0], frames[1] + 1, n)]
        lengths[0], lengths[1] = frames
    else:
        lengths = [frames] * n
    mfcc, fo, labels = planted(1 + "ABCDEFGH".index(name), n_coef, lengths, 2)
    perm = np.random.default_rng(5).permutation(n)
    train_rows, val_rows = np.sort(perm[:n_train]).astype(np.int32), np.sort(perm[n_train:]).astype(np.int32)
    rows = dict(train_rows=train_rows, val_rows=val_rows)
    seed = CASE_SEEDS[name]
    if name == "D":
        stop = dict(rows, restore_best=True, **{**base, **D_STOP, "batch_size": 32, "patience": 0})
        runs = [dict(rows, seed=seed, **base),                                                 # a full batch of 256, then 44
                dict(rows, seed=seed + 1, **{**base, "batch_size": 37, "restore_best": False}),   # sub-batches 32 + 5, last batch 4
                dict(rows, seed=seed + 2, dropout=OFF, **{**base, "batch_size": 33}),
                dict(rows, seed=seed + 3, **{**base, "batch_size": 1, "epochs": 2}),
                stop, dict(stop, restore_best=False)]
    else:
        third = {"batch_size": 1, "epochs": 2} if name in CASES_OLD else {"batch_size": ODD_BATCH[name]}
        runs = [dict(rows, seed=seed, **base),                                                 # dropout on
                dict(rows, seed=seed + 1, dropout=OFF, **base),                                  # dropout off
                dict(rows, seed=seed + 2, **{**base, **third}),                                   # batch 1 / an odd batch
                dict(rows, seed=seed + 3, **{**base, "batch_size": 256 if name in CASES_OLD else n_train + (name != "G") * 4})]   # batch >= n_train
    return {"name": name, "n_coef": n_coef, "max_frames": max_frames, "units": units, "mfcc": mfcc, "frame_offsets": fo, "labels": labels,
            "runs": runs, "train_rows": train_rows, "val_rows": val_rows}


_CACHE = {}


def case_reference(name: str) -> dict:
    """the case with its Scaler, standardised rows and the restated runs (numpy order, ascending, descending), computed once"""
    if name not in _CACHE:
        c = case(name)
        x = features(c["mfcc"], c["frame_offsets"], c["n_coef"], c["max_frames"])
        c["mean"], c["scale"] = scaler_fit(x, c["n_coef"], c["max_frames"], c["train_rows"])
        c["z"] = standardise(x, c["mean"], c["scale"], c["n_coef"], c["max_frames"])
        for fo_ in ("numpy", "asc", "desc"):
            c[fo_] = [train_run(c["z"], c["labels"], c["n_coef"], c["max_frames"], c["units"], r, fo_) for r in c["runs"]]
        c["spread"] = max(relative(a[k], d[k]) for a, d in zip(c["asc"], c["desc"]) for k in ("history", "params", "prob"))
        c["allow"] = max(4.0 * c["spread"], FLOOR)
        _CACHE[name] = c
    return _CACHE[name]
