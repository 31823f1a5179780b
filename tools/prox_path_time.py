"""A regularisation path of 8 group-lasso penalties at cfg3's shape (N = 2^20, Nf = 512, Nv = 8, 2000 iterations, tol = 0) against eight
sequential single-penalty solves: wall time of the whole call (host clock; every call ends in a device synchronise and a copy of the
parameters to the host) and the ADMM phase from timing() (HIP events of the handle's stream), one warm-up, then `--reps` repetitions.

    timeout -k 10 900 python tools/prox_path_time.py --mode both [--out profiles/prox_path_time.txt]

--mode sequential needs nothing of the path feature (it runs on a commit without it: the comparison's other side); --mode path / both
need Problem.path.  The penalties are lambda_max (largest group norm of b) times a geometric grid down to 1e-3, computed here so that
both sides solve the same eight problems; `both` also reports how far the path's columns are from the sequential solves.
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
    ap.add_argument("--mode", default="both", choices=["sequential", "path", "both"])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--nf", type=int, default=512)
    ap.add_argument("--nv", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    import lpvspectral_jl_amd as L
    from lpvspectral_jl_amd import _lib, api
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    N, Nf, Nv = 2 ** a.log2n, a.nf, a.nv
    y, X, V, w = bench.synth_signal(N, Nf, 0, torch.device("cuda", 0))
    with L.Problem.lpv(y, X, V, w, Nv) as p:                     # (untimed: the penalties)
        b = p.get_rhs()
    lmax = float(np.sqrt((b.reshape(Nf, 2 * Nv) ** 2).sum(axis=1)).max())
    lams = lmax * 1e-3 ** (np.arange(a.count) / max(a.count - 1.0, 1.0))
    gs = [L.SlicedSeparableSum.frequency_groups(l, Nf, 2 * Nv) for l in lams]
    kw = dict(iters=a.iters, tol=0.0, printerval=10 ** 9)
    sync = torch.cuda.synchronize

    def sequential():
        sync(); t0 = time.perf_counter()
        out, admm = [], 0.0
        for g in gs:
            with L.Problem.lpv(y, X, V, w, Nv) as p:
                api._admm_on_problem(p, None, g, _lib.LINEAR_LEAST_SQUARES, **kw)
                out.append(p.params(0))
                admm += p.timing()["admm_ms"]
        return time.perf_counter() - t0, admm, np.stack(out, axis=1), None

    def path():
        sync(); t0 = time.perf_counter()
        with L.Problem.lpv(y, X, V, w, Nv) as src:
            prob = L.Problem.path(src, len(gs))
        with prob:
            api._admm_on_problem(prob, None, gs, _lib.LINEAR_LEAST_SQUARES, **kw)
            P = prob.params(0).reshape(Nf * Nv, -1, order="F")
            admm = prob.timing()["admm_ms"]
            kern = prob.matvec_info()["kernel"]
        return time.perf_counter() - t0, admm, P, kern

    emit(f"# {a.label + ': ' if a.label else ''}{torch.cuda.get_device_name(0)}, N = 2^{a.log2n}, Nf = {Nf}, Nv = {Nv} (n = {2 * Nf * Nv}), {a.count} penalties "
         f"lambda_max {lmax:.6g} x 1e-3^(k/{a.count - 1}), {a.iters} iterations, tol = 0; one warm-up, then {a.reps} repetitions")
    emit(f"{'what':<28} {'rep':>3} {'whole call s':>13} {'ADMM phase ms':>14} {'ms / iteration':>15}")
    res = {}
    modes = [("sequential", sequential), ("path", path)] if a.mode == "both" else [(a.mode, sequential if a.mode == "sequential" else path)]
    for name, fn in modes:
        fn()                                                      # warm-up: code objects, allocator, the plan caches
    for r in range(a.reps):                                       # alternating
        for name, fn in modes:
            wall, admm, P, kern = fn()
            res.setdefault(name, []).append((wall, admm, P, kern))
            what = f"{a.count} sequential solves" if name == "sequential" else f"path of {a.count} ({kern})"
            emit(f"{what:<28} {r:>3} {wall:>13.4f} {admm:>14.2f} {admm / a.iters:>15.4f}")
    for name, rec in res.items():
        wl, ad = np.array([x[0] for x in rec]), np.array([x[1] for x in rec])
        emit(f"# {name}: whole call median {np.median(wl):.4f} s (min {wl.min():.4f}, max {wl.max():.4f}); ADMM phase median {np.median(ad):.2f} ms "
             f"(min {ad.min():.2f}, max {ad.max():.2f})")
    if len(res) == 2:
        ws, wp = np.median([x[0] for x in res["sequential"]]), np.median([x[0] for x in res["path"]])
        as_, ap_ = np.median([x[1] for x in res["sequential"]]), np.median([x[1] for x in res["path"]])
        emit(f"# path / sequential (this build): whole call {wp / ws:.3f}, ADMM phase {ap_ / as_:.3f}")
        Ps, Pp = res["sequential"][-1][2], res["path"][-1][2]
        for q in range(a.count):
            den = float(np.linalg.norm(Ps[:, q]))
            rel = float(np.linalg.norm(Pp[:, q] - Ps[:, q])) / den if den > 0 else float(np.linalg.norm(Pp[:, q]))
            emit(f"# column {q}: lambda {lams[q]:.6g}, non-zero parameters {int(np.count_nonzero(Pp[:, q]))} (sequential {int(np.count_nonzero(Ps[:, q]))}), "
                 f"path against its own solve rel-L2 {rel:.3e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
