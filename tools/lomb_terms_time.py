"""Time of lombscargle(..., nterms=K) (csrc/lomb_terms.hip) against the only route a user had before it existed: lombscargle(path="direct",
return_sums=True) on the concatenated grid {m f : m = 1 .. 2K} of 2K Nf frequencies, and the 2K x 2K normal equations of every (frequency,
signal) solved in numpy.

One record of N sorted non-uniform times of mean spacing 1, weights in [0.5, 2], f = (Nf + 1 .. 2 Nf) / (8 K Nf) -- in (1/8K, 1/4K]: the
highest harmonic 2K f stays within 1/2 and the lowest frequency sees hundreds of cycles, so no frequency is degenerate -- and
device-resident y, t and W on both routes.  Every configuration runs in a child process of its own under its own time limit; the tool
stops at the first child that fails.  Per configuration one warm-up of each route (the two must agree to 1e-9), then --reps repetitions;
reported is the median.
  device ms: the HIP-event times of the library's timing records (lombscargle_terms_last_timing / lombscargle_last_timing): the whole call
             (`total`), the sums kernel(s) (`sums`) and, for the new call, the epilogue that factors the systems on the device (`epi`);
  host ms:   the old route's numpy part (forming A, g, b from the sums, the batched solve, the power), by the wall clock.
The model per (sample, frequency): new = 1 sincospi + 4 (2K - 1) rotation flops + 4K + 2K ts fused multiply-adds; old = 2K sincospi +
2K (4 + 2 ts) fused multiply-adds.

    timeout -k 10 1100 python tools/lomb_terms_time.py [--out profiles/lomb_terms_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_solve(s, K, Nf, ns, fit_mean=True):
    """The old route's host part: the sums of the concatenated grid -> standard power (Nf, ns)."""
    C = np.concatenate([np.ones((1, Nf)), s["C"].reshape(2 * K, Nf)])
    S = np.concatenate([np.zeros((1, Nf)), s["S"].reshape(2 * K, Nf)])
    n = 2 * K
    A = np.empty((Nf, n, n))
    for h in range(1, K + 1):
        for j in range(1, K + 1):
            d, sg = abs(h - j), np.sign(j - h)
            A[:, 2 * h - 2, 2 * j - 2] = 0.5 * (C[d] + C[h + j])
            A[:, 2 * h - 1, 2 * j - 1] = 0.5 * (C[d] - C[h + j])
            A[:, 2 * h - 2, 2 * j - 1] = A[:, 2 * j - 1, 2 * h - 2] = 0.5 * (S[h + j] + sg * S[d])
    g = np.stack([C[1:K + 1], S[1:K + 1]], axis=1).reshape(n, Nf).T
    YC, YS = s["YC"].reshape(ns, 2 * K, Nf)[:, :K], s["YS"].reshape(ns, 2 * K, Nf)[:, :K]
    b = np.stack([YC, YS], axis=2).reshape(ns, n, Nf).transpose(2, 1, 0)       # (Nf, n, ns)
    Y, YY = s["Y"], s["YY"]
    if fit_mean:
        A = A - g[:, :, None] * g[:, None, :]
        b = b - g[:, :, None] * Y[None, None, :]
        YY = YY - Y * Y
    theta = np.linalg.solve(A, b)
    return (b * theta).sum(axis=1) / YY[None, :]


def child(N, Nf, K, ns, reps):
    import torch
    import lpvspectral_jl_amd as L
    rng = np.random.default_rng(N + ns)
    t = np.sort(rng.random(N)) * N
    y = np.cos(2 * np.pi * 0.01 * t[:, None] + np.arange(ns)[None, :]) + 0.4 * np.cos(2 * np.pi * 0.02 * t[:, None]) + rng.standard_normal((N, ns))
    W = rng.uniform(0.5, 2.0, N)
    f = np.arange(Nf + 1, 2 * Nf + 1) / (8.0 * K * Nf)
    fcat = np.concatenate([m * f for m in range(1, 2 * K + 1)])
    yd, td, Wd = (torch.tensor(a, device="cuda") for a in (y if ns > 1 else y[:, 0], t, W))

    def new():
        P = L.lombscargle(yd, td, f, W=Wd, nterms=K)
        return P.power.reshape(Nf, ns), L.lombscargle_terms_last_timing()

    def old():
        _, s = L.lombscargle(yd, td, fcat, W=Wd, path="direct", return_sums=True)
        tm = L.lombscargle_last_timing()
        t0 = time.perf_counter()
        P = host_solve(s, K, Nf, ns)
        return P, tm, (time.perf_counter() - t0) * 1e3

    Pn, _ = new()
    Po, _, _ = old()
    assert np.max(np.abs(Pn - Po)) <= 1e-9, "the two routes disagree"
    nt, nsums, nepi, ot, osums, oh = [], [], [], [], [], []
    for _ in range(reps):
        _, tm = new()
        nt.append(tm["total_ms"]); nsums.append(tm["sums_ms"]); nepi.append(tm["epilogue_ms"])
        _, tmo, h = old()
        ot.append(tmo["total_ms"]); osums.append(tmo["sums_ms"]); oh.append(h)
    med = lambda v: float(np.median(v))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "Nf": Nf, "K": K, "ns": ns, "ts": tm["ts"], "acc": tm["accumulators"], "slabs": tm["slabs"],
                      "new_total": med(nt), "new_sums": med(nsums), "new_epi": med(nepi), "old_total": med(ot), "old_sums": med(osums), "old_host": med(oh)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a configuration's child process may take")
    ap.add_argument("--samples", type=int, nargs="*", default=[1 << 14, 1 << 18, 1 << 20])
    ap.add_argument("--freqs", type=int, nargs="*", default=[512, 4096])
    ap.add_argument("--terms", type=int, nargs="*", default=[2, 4, 6])
    ap.add_argument("--child", type=int, nargs=4, default=None, metavar=("N", "Nf", "K", "ns"))
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.reps)
        return 0
    configs = [(N, Nf, K, 1) for N in a.samples for Nf in a.freqs for K in a.terms] + [(1 << 18, 4096, K, 4) for K in a.terms]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    head = False
    for N, Nf, K, ns in configs:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", str(N), str(Nf), str(K), str(ns)], timeout=a.limit,
                                 check=True, stdout=subprocess.PIPE, text=True).stdout
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            emit(f"# N = {N}, Nf = {Nf}, K = {K}, ns = {ns}: the child process failed ({type(e).__name__}); stopped here")
            return 1
        r = json.loads(out.strip().split("\n")[-1])
        if not head:
            emit(f"# lombscargle(nterms=K) against lombscargle(path='direct', return_sums=True) on the 2K Nf frequencies {{m f}} + the normal equations in numpy,")
            emit(f"# {r['device']}, device-resident y, t, W, f = (Nf + 1 .. 2 Nf) / (8 K Nf); ms, median of {a.reps} after a warm-up; device: HIP events, host: wall clock")
            emit(f"{'N':>8} {'Nf':>5} {'K':>2} {'ns':>2} {'ts':>2} {'acc':>3} {'slabs':>5} | {'new total':>9} {'sums':>8} {'epi':>6} | {'old total':>9} {'sums':>8} {'host':>8} | "
                 f"{'sums old/new':>12} {'device old/new':>14} {'all old/new':>11}")
            head = True
        emit(f"{N:>8} {Nf:>5} {K:>2} {ns:>2} {r['ts']:>2} {r['acc']:>3} {r['slabs']:>5} | {r['new_total']:>9.3f} {r['new_sums']:>8.3f} {r['new_epi']:>6.3f} | "
             f"{r['old_total']:>9.3f} {r['old_sums']:>8.3f} {r['old_host']:>8.3f} | {r['old_sums'] / r['new_sums']:>12.2f} {r['old_total'] / r['new_total']:>14.2f} "
             f"{(r['old_total'] + r['old_host']) / r['new_total']:>11.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
