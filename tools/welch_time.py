"""Time and peak device memory of welch_pgram and heatmap (csrc/melspec.hip, csrc/compress.hip) against what a user of the library did
before they existed: spectrogram followed by torch.mean(power, dim=1), and spectrogram followed by torch.log, a torch.sort of the
flattened matrix for the two thresholds, and torch.clamp.  Wall time of the whole call (device synchronised before and after), median
of --reps warm calls with the smallest and the largest beside it (the run-to-run spread); peak memory = the largest drop of the free
device memory over the call, sampled by a thread every millisecond, with the library's and torch's caches emptied first.

    timeout -k 10 900 python tools/welch_time.py [--out profiles/welch_time.txt]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATHS = {1: "LDS", 2: "4-step", 3: "Blu-LDS", 4: "Blu-4st"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def measure(fn):
        """(median ms, min ms, max ms, peak MB) of fn(): one cold call (for the peak), then reps warm ones."""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        L._lib.lib().lpvs_release_cached_memory()
        free0 = torch.cuda.mem_get_info()[0]
        low = [free0]
        stop = threading.Event()

        def watch():
            while not stop.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info()[0])
                time.sleep(0.001)
        th = threading.Thread(target=watch)
        th.start()
        r = fn()
        torch.cuda.synchronize()
        stop.set()
        th.join()
        low[0] = min(low[0], torch.cuda.mem_get_info()[0])
        del r
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            del r
        return float(np.median(ms)), min(ms), max(ms), (free0 - low[0]) / 1e6

    emit(f"# welch_pgram / heatmap, {torch.cuda.get_device_name(0)}, wall ms of the whole call, median [min .. max] of {a.reps} warm calls; "
         "peak MB = largest drop of free device memory during a cold call; window hanning")
    emit("# (a) welch_pgram against spectrogram + torch.mean(power, dim=1)")
    emit(f"{'L':>9} {'n':>8} {'nfft':>8} {'input':>6} {'path':>7} {'frames':>7} {'D':>5} {'slabs':>5} | {'welch ms':>24} {'MB':>7} | "
         f"{'spectrogram+mean ms':>24} {'MB':>7} | {'ratio':>6}")
    rng = np.random.default_rng(0)
    rows = [dict(L=2 ** 26, n=2048, nov=1024, nfft=None), dict(L=2 ** 24, n=1000, nov=500, nfft=1009),
            dict(L=2 ** 24, n=2 ** 21, nov=2 ** 20, nfft=None), dict(L=2 ** 23, n=2 ** 20, nov=2 ** 19, nfft=2 ** 20 + 1)]
    for c in rows:
        y = rng.standard_normal(c["L"])
        kw = dict(nfft=c["nfft"]) if c["nfft"] else {}
        for where in ("device", "host"):
            s = torch.from_numpy(y).cuda() if where == "device" else y

            def welch():
                return L.welch_pgram(s, c["n"], c["nov"], window=L.hanning, **kw).power

            def baseline():
                P = L.spectrogram(s, c["n"], c["nov"], window=L.hanning, **kw).power
                return torch.mean(P, dim=1) if where == "device" else torch.mean(torch.from_numpy(P), dim=1)
            w = measure(welch)
            tm = L.stft_last_timing()
            b = measure(baseline)
            nfft = int(c["nfft"] or L.nextfastfft(c["n"]))
            emit(f"{c['L']:>9} {c['n']:>8} {nfft:>8} {where:>6} {PATHS[tm['path']]:>7} {tm['frames']:>7} {tm['sum_chain']:>5} {tm['slabs']:>5} | "
                 f"{w[0]:>8.3f} [{w[1]:>6.3f} .. {w[2]:>6.3f}] {w[3]:>7.1f} | {b[0]:>8.3f} [{b[1]:>6.3f} .. {b[2]:>6.3f}] {b[3]:>7.1f} | {w[0] / b[0]:>6.3f}")
            del s
        del y
    emit("# (b) heatmap of a device-resident Spectrogram (L = 2^26, n = 2048) against torch.log + torch.sort (two thresholds) + torch.clamp")
    y = torch.from_numpy(rng.standard_normal(2 ** 26)).cuda()
    S = L.spectrogram(y, 2048, 1024, window=L.hanning)
    del y

    def heat():
        return L.heatmap(S)[2]

    def torch_heat():
        z = torch.log(S.power[1:, :])
        v = torch.sort(z.reshape(-1)).values
        m = v.numel()
        th = []
        for p in (0.005, 1.0):
            al = m * p + (1 - p)
            j = min(max(int(al), 1), m - 1)
            g = min(max(al - j, 0.0), 1.0)
            th.append(float(v[j - 1]) + g * (float(v[j]) - float(v[j - 1])))
        return torch.clamp(z, th[0], th[1])
    h = measure(heat)
    ct = L.compress_last_timing()
    t = measure(torch_heat)
    emit(f"{'values':>10} | {'heatmap ms':>24} {'MB':>7} {'passes':>6} {'skipped':>7} {'select ms':>9} {'clamp ms':>8} | {'torch ms':>24} {'MB':>7} | {'ratio':>6}")
    emit(f"{S.power[1:, :].numel():>10} | {h[0]:>8.3f} [{h[1]:>6.3f} .. {h[2]:>6.3f}] {h[3]:>7.1f} {ct['passes']:>6} {ct['digits_skipped']:>7} "
         f"{ct['select_ms']:>9.3f} {ct['clamp_ms']:>8.3f} | {t[0]:>8.3f} [{t[1]:>6.3f} .. {t[2]:>6.3f}] {t[3]:>7.1f} | {h[0] / t[0]:>6.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
