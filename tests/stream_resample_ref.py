"""The streaming resampler's definitions (include/dsp_amd.h "LIVE STREAMS AT ANOTHER RATE") restated in plain Python on
top of tests/resample_ref.py: the outputs a stream has emitted after N sample frames, what it carries, and a numpy model of push /
carry / finish in the float32 arithmetic of resample_ref.resample(dtype=np.float32)."""
import numpy as np

from tests import resample_ref as R


def taps_per_branch(up, half):
    return (2 * half + up) // up


def i_max(k, up, down, half):
    return (k * down + half) // up


def emitted(n, up, down, half):
    """K(N): the closed formula of the header"""
    if up == 1 and down == 1:
        return n
    a = n * up - 1 - half
    return a // down + 1 if a >= 0 else 0


def emitted_brute(n, up, down, half):
    """the number of outputs k whose last sample i_max(k) has arrived (i_max never decreases in k)"""
    k = 0
    while i_max(k, up, down, half) <= n - 1:
        k += 1
    return k


def carry_start(n, up, down, half):
    """the first sample frame a stream keeps after N: the first one output K(N) reads"""
    if up == 1 and down == 1:
        return n
    return max(0, i_max(emitted(n, up, down, half), up, down, half) - (taps_per_branch(up, half) - 1))


def push_plan(received, lengths, up, down, half):
    """-> out_offsets [n + 1] of one push"""
    new = [emitted(int(n0) + int(ln), up, down, half) - emitted(int(n0), up, down, half) for n0, ln in zip(received, lengths)]
    return np.concatenate([[0], np.cumsum(new)]).astype(np.int64)


def chunking(total, rng, special):
    """chunk lengths that add up to `total`: zeros, ones, the lengths in `special` (around the carry's) and random ones"""
    out, left = [], total
    while left > 0:
        kind = rng.integers(0, 4)
        c = 0 if kind == 0 else 1 if kind == 1 else int(rng.choice(special)) if kind == 2 else int(rng.integers(1, 701))
        c = min(c, left)
        out.append(c)
        left -= c
    return out


class StreamModel:
    """One stream in numpy: holds N and the carried samples [carry_start(N), N) and nothing else."""

    def __init__(self, rate_in, rate_out, dtype=np.float32):
        self.up, self.down, self.half = R.ratio(rate_in, rate_out)
        self.T = taps_per_branch(self.up, self.half)
        self.dtype = dtype
        self.h = R.taps(rate_in, rate_out).astype(dtype)
        self.n = 0
        self.carry = np.zeros(0, dtype)
        self.longest_carry = 0

    def _outputs(self, buf, c0, n_end, k0, k1):
        """outputs k0 .. k1 - 1 from buf = samples [c0, n_end): resample_ref.resample's loop, ascending input sample"""
        up, down, half, T = self.up, self.down, self.half, self.T
        k = np.arange(k0, k1, dtype=np.int64)
        a = k * down + half
        im, p = a // up, a % up
        y = np.zeros(k.size, self.dtype)
        for jj in range(T):
            i = im - (T - 1) + jj
            t = p + (T - 1 - jj) * up
            ok = (i >= 0) & (i < n_end) & (t <= 2 * half)
            if not ok.any():
                continue
            assert (i[ok] >= c0).all(), "an output reads a sample the stream no longer carries"
            y[ok] = (y[ok] + (buf[i[ok] - c0] * self.h[t[ok]]).astype(self.dtype)).astype(self.dtype)
        return y

    def push(self, chunk):
        chunk = np.asarray(chunk, self.dtype)
        if self.up == 1 and self.down == 1:
            self.n += chunk.size
            return chunk.copy()
        c0 = carry_start(self.n, self.up, self.down, self.half)
        assert self.carry.size == self.n - c0
        buf = np.concatenate([self.carry, chunk])
        n1 = self.n + chunk.size
        y = self._outputs(buf, c0, n1, emitted(self.n, self.up, self.down, self.half), emitted(n1, self.up, self.down, self.half))
        c1 = carry_start(n1, self.up, self.down, self.half)
        self.carry = buf[c1 - c0:].copy()
        self.longest_carry = max(self.longest_carry, self.carry.size)
        self.n = n1
        return y

    def finish(self):
        """the outputs a whole recording of N samples has beyond the emitted ones; the stream starts afresh"""
        if self.up == 1 and self.down == 1:
            y = np.zeros(0, self.dtype)
        else:
            c0 = carry_start(self.n, self.up, self.down, self.half)
            y = self._outputs(self.carry, c0, self.n, emitted(self.n, self.up, self.down, self.half), R.out_len(self.n, self.up, self.down))
        self.n, self.carry = 0, np.zeros(0, self.dtype)
        return y
