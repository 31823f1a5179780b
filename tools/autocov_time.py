"""Device time of autocov at arbitrary sample times (csrc/autocov.hip): generation, sort and total per case (HIP events of the library's
own stream, warm, median of 5), with device-resident outputs and separately with host outputs; the sort's bytes/s against the
~6.3 TB/s plain-read rate of the card (README); the numpy restatement (tests/_autocov_ref.py) on the same inputs where it fits.

    timeout -k 10 600 python tools/autocov_time.py [--out profiles/autocov_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

READ_RATE = 6.3e12   # B/s, plain HBM read rate of the MI355X (README)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-max-n", type=int, default=2 ** 13)
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    import _autocov_ref as R
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# autocov at arbitrary sample times, {torch.cuda.get_device_name(0)}, median of {a.reps} warm calls (HIP events)")
    emit("# pairs: kept pairs P; passes: radix passes not skipped; sort GB/s: passes * 2 * (key + value bytes) * P / sort time")
    emit(f"{'N':>6} {'t':>6} {'maxlag':>7} {'out':>6} {'pairs':>11} {'pass':>4} {'count ms':>9} {'gen ms':>8} {'sort ms':>8} "
         f"{'copy ms':>8} {'total ms':>9} {'sort GB/s':>9} {'of 6.3TB/s':>10} {'numpy s':>8}")
    rng = np.random.default_rng(0)
    for N in (2 ** 13, 2 ** 15):
        for equi in (True, False):
            t = np.arange(N, dtype=np.float64) if equi else np.sort(N * rng.random(N))
            y = rng.standard_normal(N)
            span = float(t.max() - t.min())
            for maxlag, ml_name in ((np.inf, "inf"), (0.1 * span, "10%")):
                np_s = None
                if N <= a.numpy_max_n:
                    t0 = time.perf_counter()
                    R.autofun("cov", t, y, maxlag)
                    np_s = time.perf_counter() - t0
                for out in ("device", "host"):
                    if out == "device":
                        tt, yy = torch.from_numpy(t).cuda(), torch.from_numpy(y).cuda()
                    else:
                        tt, yy = t, y
                    rec = []
                    for k in range(a.reps + 1):
                        res = L.autocov(tt, yy, maxlag)
                        del res
                        if k:
                            rec.append(L.autofun_last_timing())
                    med = {key: float(np.median([r[key] for r in rec])) for key in rec[0]}
                    P, passes = int(med["pairs"]), int(med["sort_passes"])
                    sort_bytes = passes * 2 * (8 + 8) * P
                    gbs = sort_bytes / (med["sort_ms"] * 1e-3) / 1e9 if med["sort_ms"] > 0 else 0.0
                    emit(f"{N:>6} {'equi' if equi else 'rand':>6} {ml_name:>7} {out:>6} {P:>11} {passes:>4} {med['count_ms']:>9.3f} "
                         f"{med['generate_ms']:>8.3f} {med['sort_ms']:>8.3f} {med['copy_out_ms']:>8.3f} {med['total_ms']:>9.3f} "
                         f"{gbs:>9.1f} {gbs * 1e9 / READ_RATE:>10.1%} {('%.2f' % np_s) if np_s is not None else '-':>8}")
                    del tt, yy
                    torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
