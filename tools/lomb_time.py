"""Time of lombscargle (csrc/lomb.hip) on both paths, and of the host route a user had before it existed: numpy's direct sums.

Device-resident inputs (no staging copies in the figures); per size one warm-up call per path, then --reps calls alternating between
the paths.  Reported per path: the HIP-event time of the whole call (`total`: scan, moments, sums, epilogue, copy-out of the power) and
of the sums alone (`sums`: the direct kernel and its slab tree, or all block transforms), median with the smallest and the largest
beside it.  The numpy baseline is a foreign yardstick, not the code under test: C, S, C2, S2, YC, YS by chunked matrix products in
double, wall time, at the largest N (doubling from 2^12, Nf = 512) whose run is projected to stay within about ten seconds.

    timeout -k 10 900 python tools/lomb_time.py [--out profiles/lomb_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_sums(y, t, f, chunk=16):
    w = np.full(len(t), 1.0 / len(t))
    wy = w * (y - y.mean())
    out = np.empty((6, len(f)))
    for k0 in range(0, len(f), chunk):
        ph = 2 * np.pi * np.outer(f[k0:k0 + chunk], t)
        c, s = np.cos(ph), np.sin(ph)
        out[0, k0:k0 + chunk], out[1, k0:k0 + chunk] = c @ w, s @ w
        out[2, k0:k0 + chunk], out[3, k0:k0 + chunk] = (c * c - s * s) @ w, (2 * s * c) @ w
        out[4, k0:k0 + chunk], out[5, k0:k0 + chunk] = c @ wy, s @ wy
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-seconds", type=float, default=10.0)
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)

    def record(N):
        t = np.sort(rng.random(N)) * N                                       # mean spacing 1
        y = np.cos(2 * np.pi * 0.1 * t) + rng.standard_normal(N)
        return t, y

    def grid(Nf):
        return np.arange(1, Nf + 1) * (0.5 / Nf)                             # up to the pseudo-Nyquist frequency 1/2

    def both(N, Nf):
        t, y = record(N)
        f = grid(Nf)
        td, yd = torch.from_numpy(t).cuda(), torch.from_numpy(y).cuda()
        res = {}
        for p in ("direct", "nufft"):
            L.lombscargle(yd, td, f, path=p)                                 # warm-up
            res[p] = dict(total=[], sums=[])
        for _ in range(a.reps):
            for p in ("direct", "nufft"):
                L.lombscargle(yd, td, f, path=p)
                tm = L.lombscargle_last_timing()
                assert tm["path"] == p
                res[p]["total"].append(tm["total_ms"]); res[p]["sums"].append(tm["sums_ms"]); res[p]["tm"] = tm
        return res

    def fmt(v):
        return f"{np.median(v):>9.3f} [{min(v):>8.3f} .. {max(v):>8.3f}]"

    emit(f"# lombscargle, {torch.cuda.get_device_name(0)}, one signal, unit weights, f = (1 .. Nf) / (2 Nf), device-resident t and y; HIP-event ms,")
    emit(f"# median [min .. max] of {a.reps} calls after a warm-up, the two paths alternating")
    emit(f"{'N':>8} {'Nf':>6} | {'direct total':>30} {'direct sums':>30} {'slabs':>5} | {'nufft total':>30} {'nufft sums':>30} {'blocks':>6} {'nf':>5} | "
         f"{'direct/nufft':>12}")
    rows = [(1 << 20, 512), (1 << 20, 4096), (1 << 20, 65536)] + [(1 << e, 512) for e in range(12, 20)]
    # ... and across what `auto` decides by: short grids at N = 2^20, and N Nf = 2^27, 2^28, 2^29 on long ones
    rows += [(1 << 20, 64), (1 << 20, 128), (1 << 20, 256), (1 << 22, 128), (1 << 16, 2048), (1 << 17, 2048), (1 << 18, 2048), (1 << 14, 8192), (1 << 15, 8192),
             (1 << 16, 8192)]
    for N, Nf in rows:
        r = both(N, Nf)
        d, n = r["direct"], r["nufft"]
        emit(f"{N:>8} {Nf:>6} | {fmt(d['total'])} {fmt(d['sums'])} {d['tm']['slabs']:>5} | {fmt(n['total'])} {fmt(n['sums'])} {n['tm']['blocks'][0]:>6} "
             f"{n['tm']['nf']:>5} | {np.median(d['total']) / np.median(n['total']):>12.3f}")
    emit("# the host route: numpy direct sums (C, S, C2, S2, YC, YS in double, one signal), wall seconds, Nf = 512")
    N, last = 1 << 12, None
    while True:
        t, y = record(N)
        f = grid(512)
        t0 = time.perf_counter()
        numpy_sums(y, t, f)
        last = (N, time.perf_counter() - t0)
        emit(f"{N:>8} {512:>6} | numpy {last[1]:>8.3f} s")
        if last[1] * 2 > a.host_seconds or N >= 1 << 20:
            break
        N *= 2
    r = both(last[0], 512)
    emit(f"# at N = {last[0]}, Nf = 512: numpy {last[1] * 1e3:.0f} ms, lombscargle direct {np.median(r['direct']['total']):.3f} ms, "
         f"nufft {np.median(r['nufft']['total']):.3f} ms (device-resident inputs)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
