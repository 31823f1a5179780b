"""Time of lombscargle_spectrogram (csrc/lomb.hip: the segmented kernels) against the route a user had before it existed: a loop of
lombscargle calls over the same windows.

One signal, N = 2^20 sorted non-uniform times of mean spacing 1, windows of n samples at 50 % overlap, Hann taper.  Device-resident
inputs; per shape one warm-up of each route, then --reps repetitions.  Reported per route: the device time per call -- the HIP-event
`total` of lombscargle_windows_last_timing for the one batched call, the SUM of the `total` of lombscargle_last_timing over the loop's
calls (path "direct", the weights the window's Hann taper) -- as median [min .. max], the wall time of the route beside it, and the
ratio of the device times.

    timeout -k 10 900 python tools/lomb_windows_time.py [--out profiles/lomb_windows_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    N = a.samples
    t = np.sort(rng.random(N)) * N
    y = np.cos(2 * np.pi * 0.1 * t) + rng.standard_normal(N)
    td, yd = torch.from_numpy(t).cuda(), torch.from_numpy(y).cuda()

    def fmt(v):
        return f"{np.median(v):>9.3f} [{min(v):>8.3f} .. {max(v):>8.3f}]"

    emit(f"# lombscargle_spectrogram against a loop of lombscargle, {torch.cuda.get_device_name(0)}, one signal, N = {N}, windows of n samples at 50 % overlap,")
    emit(f"# Hann taper, f = (1 .. Nf) / (2 Nf), device-resident t and y; device ms per route (HIP events), median [min .. max] of {a.reps} after a warm-up")
    emit(f"{'n':>6} {'Nf':>5} {'windows':>7} {'items':>6} | {'batched total':>30} {'moments':>8} {'sums':>8} {'epilogue':>8} {'copy':>8} {'wall':>8} | "
         f"{'loop total':>30} {'wall':>9} | {'loop/batched':>12}")
    for n in (1024, 4096, 16384):
        for Nf in (128, 512):
            f = np.arange(1, Nf + 1) * (0.5 / Nf)
            starts = np.asarray(L.Windows2(y, t, n, n // 2).offsets)
            tapers = []
            for o in starts:                                                   # the loop's weights: the same taper from time, formed once
                u = (t[o:o + n] - t[o]) / (t[o + n - 1] - t[o])
                tapers.append(torch.from_numpy(np.sin(np.pi * u) ** 2).cuda())

            def batched():
                t0 = time.perf_counter()
                S = L.lombscargle_spectrogram(yd, td, f, n=n, noverlap=n // 2, window=L.hanning)
                return S, L.lombscargle_windows_last_timing(), time.perf_counter() - t0

            def loop():
                t0, dev, cols = time.perf_counter(), 0.0, []
                for o, g in zip(starts, tapers):
                    cols.append(L.lombscargle(yd[o:o + n], td[o:o + n], f, W=g, path="direct").power)
                    dev += L.lombscargle_last_timing()["total_ms"]
                return np.stack(cols, axis=1), dev, time.perf_counter() - t0

            S, _, _ = batched()
            P, _, _ = loop()
            scale = np.max(np.abs(P))
            assert S.power.shape == P.shape and np.max(np.abs(S.power - P)) <= 1e-9 * scale, "the two routes disagree"
            bt, bw, lt, lw, tm = [], [], [], [], None
            for _ in range(a.reps):
                _, tm, w = batched()
                bt.append(tm["total_ms"]); bw.append(w * 1e3)
                _, dev, w = loop()
                lt.append(dev); lw.append(w * 1e3)
            emit(f"{n:>6} {Nf:>5} {tm['windows']:>7} {tm['items']:>6} | {fmt(bt)} {tm['moments_ms']:>8.3f} {tm['sums_ms']:>8.3f} {tm['epilogue_ms']:>8.3f} "
                 f"{tm['copy_ms']:>8.3f} {np.median(bw):>8.1f} | {fmt(lt)} {np.median(lw):>9.1f} | {np.median(lt) / np.median(bt):>12.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
