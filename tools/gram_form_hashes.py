#!/usr/bin/env python3
"""One line per constructor path: SHA-256 of G, SHA-256 of b, and timing()'s gram_form / gram_stage / gram_ksplit -- the smallest shape
that reaches each path of the problem constructors (csrc/api.hip, csrc/gram_form_plan.h) and of the window engine's form decision.
Two builds of the library compute the same thing exactly when their outputs are identical:

    LPVS_LIBRARY=/path/to/other/liblpvspectral.so tools/gram_form_hashes.py > a.txt;  tools/gram_form_hashes.py > b.txt;  cmp a.txt b.txt

Inputs are fixed (seeded); nothing in the output depends on time."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lpvspectral_jl_amd as L

D = 0.25


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def report(name, p):
    G, _ = p.get_gram()
    b = p.get_rhs()
    tm = p.timing()
    print(f"{name:34s} G {sha(G)} b {sha(b)} form {tm['gram_form']} stage {tm['gram_stage']} ksplit {tm['gram_ksplit']}", flush=True)


def signal(N, seed=0, ns=1):
    rng = np.random.default_rng(seed)
    X = np.sort(10 * rng.random(N))
    V = rng.random(N)
    Y = rng.standard_normal((N, ns))
    return (Y[:, 0] if ns == 1 else Y), X, V


def lpv_cases():
    w = D * np.arange(1, 9)
    y, X, V = signal(4096)
    with L.Problem.lpv(y, X, V, w, 2) as p:
        report("lpv N=4096 ap-nufft", p)
    with L.default_options(slot_sums="direct"), L.Problem.lpv(y, X, V, w, 2) as p:
        report("lpv N=4096 slot_sums=direct", p)
    with L.Problem.lpv(y, X, V, D / 2 + D * np.arange(8), 2) as p:
        report("lpv N=4096 rhs off the grid", p)
    yn = y.copy(); yn[100] = np.nan
    with L.Problem.lpv(yn, X, V, w, 2) as p:
        report("lpv N=4096 NaN in y", p)
    with L.Problem.lpv(y, X, V, w, 2, True, True) as p:
        report("lpv N=4096 coulomb", p)
    Y3, _, _ = signal(4096, ns=3)
    with L.Problem.lpv_multi(Y3, X, V, w, 2) as p:
        report("lpv N=4096 ns=3", p)
    with L.Problem.lpv_rows(y[:2048], X[:2048], V[:2048], w, 2, L.lpv_ranges(X, V)) as p:
        report("lpv rows [0, 2048) of 4096", p)
    y, X, V = signal(600, 1)
    wp = w.copy(); wp[3] += 1e-3
    with L.Problem.lpv(y, X, V, wp, 2) as p:
        report("lpv N=600 perturbed grid", p)
    with L.Problem.lpv(y, X, V, wp, 1) as p:
        report("lpv N=600 Nv=1", p)
    with L.default_options(gram_form="kr"), L.Problem.lpv(y, X, V, w, 2) as p:
        report("lpv N=600 gram_form=kr", p)
    Y3, _, _ = signal(600, 1, ns=3)
    with L.Problem.lpv_multi(Y3, X, V, wp, 2) as p:
        report("lpv N=600 perturbed grid ns=3", p)
    # a float-rounded grid: admitted through the _f32 entry point, not through the _f64 one
    y, X, V = signal(4096, 2)
    X = 100 * X                                      # residual phases of 1e-5: beyond the double-precision bound, within a float ulp
    w32 = (0.1 * np.arange(1, 9)).astype(np.float32)
    with L.Problem.lpv(y.astype(np.float32), X.astype(np.float32), V.astype(np.float32), w32, 2) as p:
        report("lpv_f32 float-rounded grid", p)
    with L.Problem.lpv(y.astype(np.float32).astype(float), X.astype(np.float32).astype(float), V.astype(np.float32).astype(float), w32.astype(float), 2) as p:
        report("lpv_f64 the same grid", p)


def fourier_cases():
    rng = np.random.default_rng(3)
    N = 4096
    t = np.sort(10 * rng.random(N)); y = rng.standard_normal(N); W = rng.random(N)
    f = 0.5 * np.arange(1, 9)
    with L.Problem.fourier(y, t, f) as p:
        report("fourier N=4096 progression", p)
    with L.Problem.fourier(y, t, f, W) as p:
        report("fourier N=4096 progression, W", p)
    with L.Problem.fourier(y, t, 0.5 * np.arange(8)) as p:
        report("fourier N=4096 zero frequency", p)
    fp = f.copy(); fp[3] += 1e-3
    with L.Problem.fourier(y, t, fp) as p:
        report("fourier N=4096 perturbed grid", p)
    A = rng.standard_normal((600, 12)); yd = rng.standard_normal(600)
    with L.Problem.dense(A, yd) as p:
        report("dense m=600 n=12", p)
    G = A.T @ A
    with L.Problem.gram(G, A.T @ yd) as p:
        report("gram n=12", p)


def window_cases():
    rng = np.random.default_rng(4)
    n, Lw = 2048, 3 * 2048
    t = np.sort(30 * rng.random(Lw)); y = rng.standard_normal(Lw)
    f = 0.25 * np.arange(1, 33)                      # 32 frequencies on a progression: 72 slots in the merged layout
    for name, opts in (("windows n=2048 Nf=32", {}), ("windows n=2048 Nf=32 direct", dict(slot_sums="direct"))):
        with L.default_options(**opts):
            x, S, its = L.windowpsd_sparse_batched(y, t, f, n, 0, None, λ=0.5, iters=20, tol=0.0)
        print(f"{name:34s} x {sha(x)} S {sha(S)} form {L.windowpsd_last_timing()['gram_form']}", flush=True)


if __name__ == "__main__":
    lpv_cases()
    fourier_cases()
    window_cases()
