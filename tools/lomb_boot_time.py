"""Time of lombscargle_bootstrap (csrc/lomb_boot.hip) against the route a user had before it existed: the resamples drawn on the host with
bootstrap_indices, uploaded as signals, lombscargle(path="direct") over them in groups of signals, the maxima taken in numpy.

One record of N sorted non-uniform times of mean spacing 1, weights in [0.5, 2], f = (1 .. Nf) / (2 Nf), B resamples of seed 0.  Host
inputs on both routes (the old route has to upload its B x N matrix; the new call uploads the record).  Per shape one warm-up of each
route, then --reps repetitions.  Reported: the device time -- the HIP-event `total` of lombscargle_bootstrap_last_timing, for both
instantiations of the kernel (TS = 16 and, through the experiment knob, TS = 8), and the SUM of the `total` of lombscargle_last_timing
over the old route's calls -- as median [min .. max], the wall time beside it, and the ratio old / new of the device times.  The old
route's indices and gathered matrix are formed once per (N, B) outside the timed region; the seconds that took are listed (`draw`).

    timeout -k 10 900 python tools/lomb_boot_time.py [--out profiles/lomb_boot_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("LPVS_EXPERIMENTS", "1")                                # (the TS knob is an experiment knob)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--group", type=int, default=128, help="signals per lombscargle call of the old route")
    ap.add_argument("--samples", type=int, nargs="*", default=[1 << 12, 1 << 14, 1 << 16])
    ap.add_argument("--freqs", type=int, nargs="*", default=[512, 4096])
    ap.add_argument("--resamples", type=int, nargs="*", default=[64, 1024])
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        return f"{np.median(v):>9.3f} [{min(v):>8.3f} .. {max(v):>8.3f}]"

    emit(f"# lombscargle_bootstrap against resamples drawn on the host + lombscargle(path='direct') in groups of {a.group} signals + maxima in numpy,")
    emit(f"# {torch.cuda.get_device_name(0)}, host inputs, f = (1 .. Nf) / (2 Nf); device ms (HIP events), median [min .. max] of {a.reps} after a warm-up; wall ms: median")
    emit(f"{'N':>6} {'Nf':>5} {'B':>5} {'chunks':>6} | {'new (TS 16) total':>30} {'shared':>7} {'moments':>7} {'sums':>8} {'epilogue':>8} {'copy':>6} {'wall':>8} | "
         f"{'new (TS 8) total':>30} {'sums':>8} | {'old route total':>30} {'wall':>9} {'draw s':>6} | {'old/new':>7}")
    for N in a.samples:
        rng = np.random.default_rng(N)
        t = np.sort(rng.random(N)) * N
        y = np.cos(2 * np.pi * 0.1 * t) + rng.standard_normal(N)
        W = rng.uniform(0.5, 2.0, N)
        for B in a.resamples:
            t0 = time.perf_counter()
            Ys = np.empty((N, B), order="F")                                    # the old route's B x N matrix, column b = y[pi_b]
            for b0 in range(0, B, 64):
                nb = min(64, B - b0)
                Ys[:, b0:b0 + nb] = y[L.bootstrap_indices(N, nb, seed=0, row0=b0)].T
            draw = time.perf_counter() - t0
            for Nf in a.freqs:
                f = np.arange(1, Nf + 1) * (0.5 / Nf)

                def new(ts):
                    os.environ["LPVS_LOMB_BOOT_TS"] = str(ts)
                    t0 = time.perf_counter()
                    M = L.lombscargle_bootstrap(y, t, f, W=W, B=B, seed=0)
                    w = time.perf_counter() - t0
                    return M, L.lombscargle_bootstrap_last_timing(), w

                def old():
                    t0, dev, M = time.perf_counter(), 0.0, []
                    for b0 in range(0, B, a.group):
                        P = L.lombscargle(Ys[:, b0:b0 + a.group], t, f, W=W, path="direct").power
                        dev += L.lombscargle_last_timing()["total_ms"]
                        M.append(P.max(axis=0))
                    return np.concatenate(M), dev, time.perf_counter() - t0

                M16, tm, _ = new(16)
                M8, tm8, _ = new(8)
                Mo, _, _ = old()
                assert tm["ts"] == 16 and tm8["ts"] == 8
                for M in (M16, M8):
                    assert M.shape == Mo.shape and np.max(np.abs(M - Mo)) <= 1e-9 * np.max(np.abs(Mo)), "the two routes disagree"
                nt, nw, n8, ot, ow = [], [], [], [], []
                for _ in range(a.reps):
                    _, tm, w = new(16)
                    nt.append(tm["total_ms"]); nw.append(w * 1e3)
                    _, tm8, _ = new(8)
                    n8.append(tm8["total_ms"])
                    _, dev, w = old()
                    ot.append(dev); ow.append(w * 1e3)
                emit(f"{N:>6} {Nf:>5} {B:>5} {tm['chunks']:>6} | {fmt(nt)} {tm['shared_ms']:>7.3f} {tm['moments_ms']:>7.3f} {tm['sums_ms']:>8.3f} {tm['epilogue_ms']:>8.3f} "
                     f"{tm['copy_ms']:>6.3f} {np.median(nw):>8.1f} | {fmt(n8)} {tm8['sums_ms']:>8.3f} | {fmt(ot)} {np.median(ow):>9.1f} {draw:>6.1f} | "
                     f"{np.median(ot) / np.median(nt):>7.2f}")
    os.environ.pop("LPVS_LOMB_BOOT_TS", None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
