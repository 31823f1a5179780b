"""Device time of spectrogram / melspectrogram / mfcc (csrc/melspec.hip): HIP events of the library's own stream, warm, median of 5.
Per case: the host setup (tables, band ranges, uploads), the device time (FFTs and epilogue), the copy-out, the input read rate against the ~6.3 TB/s plain-read rate of the card (README; the
signal's bytes / kernel time -- overlapping frames are re-read from L2 / MALL, not counted) and the f64 rate counted as
2.5 nfft log2(nfft) flops per frame.

    timeout -k 10 900 python tools/melspec_time.py [--out profiles/melspec_time.txt]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_RATE = 6.3e12   # B/s, plain HBM read rate of the MI355X (README)
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

    emit(f"# spectrogram / melspectrogram / mfcc, {torch.cuda.get_device_name(0)}, median of {a.reps} warm calls (HIP events)")
    emit("# setup: host tables, band ranges, uploads; device: FFTs + epilogue; in GB/s: signal bytes / device time; GFLOP/s: 2.5 nfft log2(nfft)"
         " per frame / device time; window hanning")
    emit(f"{'L':>9} {'n':>8} {'nfft':>8} {'kind':>5} {'nmels':>5} {'dtype':>5} {'out':>6} {'path':>7} {'frames':>7} {'pairs/WG':>8} "
         f"{'setup ms':>8} {'dev ms':>8} {'copy ms':>8} {'total ms':>9} {'in GB/s':>8} {'of 6.3TB/s':>10} {'GFLOP/s':>8}")
    rng = np.random.default_rng(0)
    cases = []
    for kind in ("power", "mel", "mfcc"):
        cases.append(dict(L=2 ** 26, n=2048, nov=1024, nfft=None, kind=kind, nmels=128, dt="f64", out="device"))
    cases += [
        dict(L=2 ** 26, n=1024, nov=512, nfft=None, kind="mel", nmels=64, dt="f64", out="device"),
        dict(L=2 ** 24, n=2 ** 21, nov=2 ** 20, nfft=None, kind="mel", nmels=128, dt="f64", out="device"),
        dict(L=2 ** 24, n=1000, nov=500, nfft=1009, kind="mel", nmels=128, dt="f64", out="device"),
        dict(L=2 ** 23, n=2 ** 20, nov=2 ** 19, nfft=2 ** 20 + 1, kind="power", nmels=128, dt="f64", out="device"),
        dict(L=2 ** 26, n=2048, nov=1024, nfft=None, kind="mel", nmels=128, dt="f32", out="device"),
        dict(L=2 ** 26, n=2048, nov=1024, nfft=None, kind="power", nmels=128, dt="f64", out="host"),
        dict(L=2 ** 26, n=2048, nov=1024, nfft=None, kind="mel", nmels=128, dt="f64", out="host"),
    ]
    for c in cases:
        y = rng.standard_normal(c["L"]).astype(np.float32 if c["dt"] == "f32" else np.float64)
        s = torch.from_numpy(y).cuda() if c["out"] == "device" else y
        kw = dict(nfft=c["nfft"]) if c["nfft"] else {}
        rec = []
        for k in range(a.reps + 1):
            if c["kind"] == "power":
                r = L.spectrogram(s, c["n"], c["nov"], window=L.hanning, **kw)
            elif c["kind"] == "mel":
                r = L.melspectrogram(s, c["n"], c["nov"], nmels=c["nmels"], **kw)
            else:
                r = L.mfcc(s, c["n"], c["nov"], nmels=c["nmels"], **kw)
            del r
            if k:
                rec.append(L.stft_last_timing())
        med = {key: float(np.median([r[key] for r in rec])) for key in rec[0]}
        nfft = int(c["nfft"] or L.nextfastfft(c["n"]))
        frames = int(med["frames"])
        gbs = y.nbytes / (med["fft_ms"] * 1e-3) / 1e9
        gfl = 2.5 * nfft * math.log2(nfft) * frames / (med["fft_ms"] * 1e-3) / 1e9
        emit(f"{c['L']:>9} {c['n']:>8} {nfft:>8} {c['kind']:>5} {c['nmels'] if c['kind'] != 'power' else '-':>5} {c['dt']:>5} {c['out']:>6} "
             f"{PATHS[int(med['path'])]:>7} {frames:>7} {int(med['pairs_per_workgroup']):>8} {med['setup_ms']:>8.3f} {med['fft_ms']:>8.3f} {med['copy_out_ms']:>8.3f} "
             f"{med['total_ms']:>9.3f} {gbs:>8.1f} {gbs * 1e9 / READ_RATE:>10.1%} {gfl:>8.1f}")
        del s, y
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
