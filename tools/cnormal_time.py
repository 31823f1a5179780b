"""Device time of the ComplexNormal path (csrc/cnormal.hip): factor / sample / bands of schedfunc at (Nf, Nv) = (12, 50), (128, 8),
(512, 8) with nMC = 5000 (HIP events of the library's own stream, warm, median of 5), the Cholesky's fraction of the f64 matrix-core
issue ceiling (66.5 TFLOP/s, measured by tools/mfma_f64_peak.hip), the band kernel's cells/s, and the numpy restatement
(tests/_cnormal_ref.py) on the same inputs where its FB array fits.  The covariance is synthetic (a rank-64 term plus a ridge):
none of the kernels' work depends on the values.

    timeout -k 10 900 python tools/cnormal_time.py [--out profiles/cnormal_time.txt]

--normals: instead, the largest error of the device normals against the restatement in long double over 10^7 elements, in units of
u * r (r = sqrt(-2 ln u1), the draw's radius): the figure the tolerance of tests/test_gpu_cnormal.py is twice of.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_F64_PEAK = 66.5e12   # FLOP/s, issue ceiling of v_mfma_f64_16x16x4_f64 (tools/mfma_f64_peak.hip, DESIGN_APPENDIX.md)


def normals_error(L, R, emit):
    u = 2.0 ** -53
    worst, total, where = 0.0, 0, None
    rows, cols = 20000, 50
    for blk in range(10):                                   # 10 x 10^6 elements, distinct seeds and row offsets
        seed, row0 = 1000 + blk, blk * 123457
        got = L.randn(rows, cols, seed=seed, row0=row0)
        ref, rad = R.randn(seed, row0, rows, cols, dtype=np.longdouble)
        err = np.abs(got - ref) / (u * rad)
        k = np.unravel_index(int(np.argmax(err)), err.shape)
        if float(err[k]) > worst:
            worst, where = float(err[k]), (seed, int(row0 + k[0]), int(k[1]), float(got[k]))
        total += got.size
    emit(f"# device normals against the long-double restatement: max |dz| / (u r) = {worst:.3f} over {total} elements "
         f"(seed, row, column, value of the worst: {where})")
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--numpy-max-cells", type=int, default=128 * 100)
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    import _cnormal_ref as R
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.normals:
        normals_error(L, R, emit)
    else:
        emit(f"# ComplexNormal / schedfunc, {torch.cuda.get_device_name(0)}, nMC = 5000, median of {a.reps} warm calls (HIP events)")
        emit("# chol: (2n)^3 / 3 flop over the factor time, against the 66.5 TFLOP/s f64 matrix-core issue ceiling; sample: nMC (2n)^2 flop")
        emit("# total: factor + sample + bands; wall: one schedfunc call from numpy inputs (uploads the host covariance); wall dev: the covariance is a device tensor")
        emit(f"{'Nf':>4} {'Nv':>3} {'2n':>5} {'factor ms':>10} {'chol TF/s':>9} {'of peak':>8} {'sample ms':>10} {'sample TF/s':>11} "
             f"{'bands ms':>9} {'cells/s':>10} {'total ms':>9} {'wall ms':>9} {'wall dev':>9} {'numpy s':>8}")
        rng = np.random.default_rng(0)
        nMC = 5000
        for Nf, Nv in ((12, 50), (128, 8), (512, 8)):
            n = Nf * Nv
            B = rng.standard_normal((2 * n, 64))
            Sigma = (B @ B.T) / 64 * 1e-2 + 1e-3 * np.eye(2 * n)
            x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            V = np.linspace(0, 1, 500)
            w = 2 * np.pi * np.arange(1, Nf + 1, dtype=np.float64)
            se = L.SpectralExt(None, None, V, w, Nv, 0.0, False, True, x, Sigma)
            rec, wall = [], []
            for k in range(a.reps + 1):
                t0 = time.perf_counter()
                sf = L.schedfunc(se, nMC=nMC, seed=k)
                t1 = time.perf_counter()
                if k:
                    rec.append(L.cn_last_timing()); wall.append(t1 - t0)
            med = {key: float(np.median([r[key] for r in rec])) for key in rec[0]}
            sed = L.SpectralExt(None, None, V, w, Nv, 0.0, False, True, x, torch.from_numpy(Sigma).cuda())   # Σ already on the device
            wall_dev = []
            for k in range(a.reps + 1):
                t0 = time.perf_counter()
                sf = L.schedfunc(sed, nMC=nMC, seed=k)
                wall_dev.append(time.perf_counter() - t0)
            del sed
            np_s = None
            if Nf * 100 <= a.numpy_max_cells:
                Rn = L.randn(nMC, 2 * n, seed=0)
                t0 = time.perf_counter()
                U = np.linalg.cholesky(Sigma).T
                R.schedfunc(x, Sigma, V, w, Nv, True, False, R=Rn, U=U, nMC=nMC)
                np_s = time.perf_counter() - t0
            chol = (2 * n) ** 3 / 3 / (med["factor_ms"] * 1e-3)
            samp = nMC * (2 * n) ** 2 / (med["sample_ms"] * 1e-3)      # the triangular product: 2 * nMC * (2n)^2 / 2
            emit(f"{Nf:>4} {Nv:>3} {2 * n:>5} {med['factor_ms']:>10.3f} {chol / 1e12:>9.3f} {chol / MFMA_F64_PEAK:>8.2%} {med['sample_ms']:>10.3f} "
                 f"{samp / 1e12:>11.3f} {med['bands_ms']:>9.3f} {med['cells'] / (med['bands_ms'] * 1e-3):>10.3e} "
                 f"{med['factor_ms'] + med['total_ms']:>9.3f} {float(np.median(wall)) * 1e3:>9.1f} {float(np.median(wall_dev[1:])) * 1e3:>9.1f} {('%.2f' % np_s) if np_s is not None else '-':>8}")
            del sf
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if os.path.exists(a.out) and a.normals else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
