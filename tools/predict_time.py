"""Time of predict (csrc/eval.hip) on its two paths -- the direct sums and the type-2 non-uniform FFT -- at the benchmark's shape
(cfg3: M = 2^20 samples, Nf = 512, Nv = 8; 1 and 8 coefficient columns), over M = 2^10 .. 2^20 to show where the paths cross (also with
a short grid, Nf = 32), and, for
context, of the only route there was before: lpv_regressor followed by a host product, at M = 2^16 where the regressor (4.3 GB) still fits.

X, V and the output are device tensors (no copies of the samples in the timed call).  Wall ms of the whole call, device synchronised before
and after: median [min .. max] of --reps warm calls; the phases are the library's own device events of the last call
(lpvs_eval_last_timing).  Inputs: bench.py's cfg3 generator (w = 2 pi (1 .. Nf) 25 / Nf, X sorted uniform on [0, M / 50)).

    timeout -k 10 600 python tools/predict_time.py [--out profiles/predict_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NF, NV = 512, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log2m", type=int, default=20, help="largest M (the sweep starts at 2^10)")
    a = ap.parse_args()
    import torch
    import lpvspectral_jl_amd as L
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def inputs(M, nc, Nf=NF, seed=0):
        g = torch.Generator(device="cuda").manual_seed(0x1B5EC + 3 + seed)
        X = torch.sort(torch.rand(M, dtype=torch.float64, device="cuda", generator=g) * (10.0 * M / 500)).values.contiguous()
        V = torch.linspace(0, 1, M, dtype=torch.float64, device="cuda")
        w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
        rng = np.random.default_rng(seed)
        P = rng.standard_normal((Nf * NV, nc)) + 1j * rng.standard_normal((Nf * NV, nc))
        se = L.SpectralExt(None, X, V, w, NV, 1.0, False, True, P if nc > 1 else P[:, 0], None)
        return se, torch.empty(M * nc, dtype=torch.float64, device="cuda")

    def measure(fn, reps):
        fn()                                                              # warm: code objects, the allocator's blocks
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), min(ms), max(ms)

    emit(f"# predict, {torch.cuda.get_device_name(0)}; LPV model Nf = {NF}, Nv = {NV}; wall ms of the whole call = median [min .. max] of {a.reps} warm "
         "calls (it includes the two range reductions over the training record); phases = device events of the last call")
    emit("# (a) the benchmark's shape")
    head = (f"{'M':>8} {'nc':>3} {'path':>6} {'nf':>5} {'twin':>4} | {'wall ms':>26} | {'stage':>7} {'grids':>7} {'eval':>8} {'copy':>7} {'total':>8} | "
            f"{'samples/s (eval)':>16}")
    emit(head)

    def row(M, nc, path, reps, Nf=NF):
        se, out = inputs(M, nc, Nf)
        w = measure(lambda: L.predict(se, path=path, out=out), reps)
        tm = L.eval_last_timing()
        assert tm["path"] == path
        emit(f"{M:>8} {nc:>3} {path:>6} {tm['nf']:>5} {int(tm['twin']):>4} | {w[0]:>9.3f} [{w[1]:>6.3f} .. {w[2]:>6.3f}] | {tm['stage_ms']:>7.3f} {tm['grid_ms']:>7.3f} "
             f"{tm['eval_ms']:>8.3f} {tm['copy_ms']:>7.3f} {tm['total_ms']:>8.3f} | {M / (tm['eval_ms'] * 1e-3):>16.3e}")
        return w[0], tm

    M = 1 << a.log2m
    for nc in (1, 8):
        for path in ("direct", "nufft"):
            row(M, nc, path, a.reps)
    emit("# (b) both paths over M, one coefficient column: where they cross (device total = stage + grids + eval + copy)")
    emit(head)
    cross = None
    for lg in range(10, a.log2m + 1):
        d = row(1 << lg, 1, "direct", a.reps)
        n = row(1 << lg, 1, "nufft", a.reps)
        if cross is None and n[1]["total_ms"] < d[1]["total_ms"]:
            cross = lg
    emit(f"# the type-2 path's device total is below the direct path's from M = 2^{cross} on" if cross is not None
         else "# the type-2 path's device total is never below the direct path's in this range")
    emit("# (b') the same with a short frequency grid, Nf = 32 (nf = 256): the direct path's work is 16 times smaller, the type-2 path's launches are not")
    emit(head)
    for lg in range(10, min(a.log2m, 18) + 1, 2):
        row(1 << lg, 1, "direct", a.reps, 32)
        row(1 << lg, 1, "nufft", a.reps, 32)
    emit("# (c) context, the route before predict existed: lpv_regressor (device, copied to the host) + a host product, M = 2^16 (4.3 GB regressor)")
    Mc = 1 << min(16, a.log2m)
    se, out = inputs(Mc, 1)
    Xh, Vh = se.X.cpu().numpy(), se.V.cpu().numpy()
    coef = np.concatenate([se.x.real, se.x.imag])

    def old_route():
        return L.lpv_regressor(Xh, Vh, se.w, NV, True, False, permuted=False) @ coef
    o = measure(old_route, 2)
    seh = L.SpectralExt(None, Xh, Vh, se.w, NV, 1.0, False, True, se.x, None)
    p = measure(lambda: L.predict(seh, path="auto"), a.reps)
    emit(f"{'M':>8} | {'regressor + host product ms':>30} | {'predict (host arrays, auto) ms':>32}")
    emit(f"{Mc:>8} | {o[0]:>10.1f} [{o[1]:>7.1f} .. {o[2]:>7.1f}] | {p[0]:>12.3f} [{p[1]:>6.3f} .. {p[2]:>6.3f}]")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
