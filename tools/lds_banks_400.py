#!/usr/bin/env python3
"""LDS bank model of mfcc400_kernel's per-frame FFT accesses (same rules as tools/lds_banks_2048.py: ds_read_b64 = 2 groups of 32 lanes,
bank (a/4) mod 64; ds_write_b64 = 4 groups of 16, bank (a/4) mod 32; ds_read_b32 / ds_write_b32 = 2 x 32, mod 32; a group costs one
cycle per distinct address on its busiest bank).  Prints cycles per access pattern against the conflict-free count.  The image index
ZI is the kernel's (mfcc400_kernel.hip); another one can be given as a lambda on the command line to compare."""
import sys

from lds_banks_2048 import cost


def main():
    ZI = (lambda i: i) if len(sys.argv) < 2 else eval(sys.argv[1])
    rows = []

    def acc(name, fn, n, width, write):
        c = i = 0
        for t in n:
            idx = [fn(l, t) for l in range(64)]
            cc, _ = cost([width * x if x is not None else None for x in idx], width, write)
            c += cc
            g = 16 if (write and width == 8) else 32      # groups without an active lane cost nothing
            i += sum(any(x is not None for x in idx[a:a + g]) for a in range(0, 64, g))
        rows.append((name, c, i))

    on = lambda l, n, v: v if l < n else None
    acc("pass0 write zbuf[ZI(5 j + q)], j < 40", lambda l, q: on(l, 40, ZI(5 * l + q)), range(5), 8, True)
    acc("pass1 read  zbuf[ZI(j + 40 t)], j < 40", lambda l, t: on(l, 40, ZI(l + 40 * t)), range(5), 8, False)
    acc("pass1 write zbuf[ZI(5 (j - k) + k + 5 q)], k = j % 5", lambda l, q: on(l, 40, ZI(5 * (l - l % 5) + l % 5 + 5 * q)), range(5), 8, True)
    acc("pass2 read  zbuf[ZI(j + 25 t)], j < 25", lambda l, t: on(l, 25, ZI(l + 25 * t)), range(8), 8, False)
    acc("pass2 write zbuf[ZI(j + 25 q)], j < 25", lambda l, q: on(l, 25, ZI(l + 25 * q)), range(8), 8, True)
    acc("untangle read zbuf[ZI(k)], k = l + 64 t < 100", lambda l, t: on(l + 64 * t, 100, ZI(l + 64 * t)), range(2), 8, False)
    acc("untangle read zbuf[ZI(200 - k)]", lambda l, t: on(l + 64 * t, 100, ZI(200 - l - 64 * t)), range(2), 8, False)
    acc("pbuf write [k]", lambda l, t: on(l + 64 * t, 100, l + 64 * t), range(2), 4, True)
    acc("pbuf write [200 - k]", lambda l, t: on(l + 64 * t, 100, 200 - l - 64 * t), range(2), 4, True)
    tot = sum(r[1] for r in rows)
    ideal = sum(r[2] for r in rows)
    for name, c, i in rows:
        print(f"{name:60s} {c:4d} cycles (conflict-free {i})")
    print(f"{'total (FFT + untangle + power spectrum)':60s} {tot:4d} cycles (conflict-free {ideal})")


if __name__ == "__main__":
    main()
