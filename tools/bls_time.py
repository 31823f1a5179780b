"""Time of bls (csrc/bls.hip) against the route a user had before it existed: a chunked PyTorch evaluation of the same definition on the
device -- fold, scatter_add_ into float64 histograms, cumsum, every box, arg-max -- a chunk of frequencies at a time.

One record of N non-uniform times (multiples of 2^-10, mean spacing 1, in random order), weights in [0.5, 2], one signal: noise of
sigma 1 and a dip of depth 1 lasting 3 % of the period 1 / 0.1171875; Nf frequencies over [0.05, 0.5], multiples of 2^-20: every product
f t is exact in double, so both routes fold every sample into the same bin and have to agree.  q = (0.01, 0.1).  Device-resident y, t
and W on both routes.  Before anything is timed the PyTorch route is held to tests/_bls_ref.py: bls_ref_ld (long double, every box
summed bin by bin) on the CPU.  Every configuration runs in a child process of its own under its own time limit; the tool stops at the
first child that fails.  Per configuration one warm-up of each route (the powers must agree to 1e-9), then --reps repetitions; reported
is the median.
  new:   the HIP-event times of bls_last_timing: the whole call (`total`), the scan and the moments (`scan`), the maxima and the
         quantisation (`quant`), fold and search (`search`).
  torch: torch.cuda events around the whole evaluation.  Where Nf N is more than --dense-limit elements it is run on the first `sub`
         frequencies only and the time is scaled by Nf / sub (its chunks are independent and equal): the column `sub` says so.
The cost model of the new call: one fold and 1 + ts LDS atomic adds (plus the count) per (sample, frequency), 2 nbins widths divisions per
frequency.  `ns/pair` is the fold-and-search time per (sample, frequency) in nanoseconds, `ns/box` the same time per box tried.

    timeout -k 10 1100 python tools/bls_time.py [--out profiles/bls_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q = (0.01, 0.1)


def widths(nbins):
    return max(1, int(np.floor(Q[0] * nbins))), min(nbins // 2, int(np.ceil(Q[1] * nbins)))


def torch_bls(torch, y, t, W, f, nbins, kmin, kmax, chunk):
    """-> power (standard), start, width per frequency; everything on the device of y.  Unit min_count, dips only."""
    w = W / W.sum()
    wy = w * (y - (w * y).sum())
    YY = (wy * (y - (w * y).sum())).sum()
    ones = torch.ones_like(w)
    power, start, width = [], [], []
    for k0 in range(0, len(f), chunk):
        fd = torch.as_tensor(f[k0:k0 + chunk], device=y.device)
        ph = fd[:, None] * t[None, :]
        ph = ph - torch.floor(ph)
        bins = torch.clamp((ph * nbins).long(), max=nbins - 1)
        H = torch.zeros((3, len(fd), nbins), dtype=torch.float64, device=y.device)
        for row, v in enumerate((w, wy, ones)):
            H[row].scatter_add_(1, bins, v[None, :].expand(len(fd), -1))
        P = torch.cumsum(torch.cat([H, H], dim=2), dim=2)
        P = torch.cat([torch.zeros_like(P[..., :1]), P], dim=2)
        R, S = H[0].sum(dim=1, keepdim=True), H[1].sum(dim=1, keepdim=True)
        best = torch.full((len(fd),), -1.0, dtype=torch.float64, device=y.device)
        bk = torch.zeros(len(fd), dtype=torch.long, device=y.device)
        bb = torch.zeros_like(bk)
        for k in range(kmin, kmax + 1):
            r, s, cnt = (P[row][:, k:k + nbins] - P[row][:, :nbins] for row in range(3))
            rc, sc = R - r, S - s
            ok = (cnt >= 1) & (len(t) - cnt >= 1) & (r > 0) & (rc > 0)
            rs, rcs = torch.where(ok, r, torch.ones_like(r)), torch.where(ok, rc, torch.ones_like(rc))
            ok &= s / rs < sc / rcs
            d = torch.where(ok, s * s / rs + sc * sc / rcs - S * S / R, torch.full_like(r, -1.0))
            v, i = d.max(dim=1)
            better = v > best
            best, bk, bb = torch.where(better, v, best), torch.where(better, torch.full_like(bk, k), bk), torch.where(better, i, bb)
        power.append(torch.clamp(best, min=0.0) / YY)
        start.append(bb); width.append(bk)
    return torch.cat(power), torch.cat(start), torch.cat(width)


def record(N, Nf):
    rng = np.random.default_rng(N)
    t = rng.permutation(np.round((np.arange(N) + rng.random(N)) * 1024) / 1024)
    y = rng.standard_normal(N)
    y[np.mod(0.1171875 * t, 1.0) < 0.03] -= 1.0
    W = rng.uniform(0.5, 2.0, N)
    f = np.round(np.linspace(0.05, 0.5, Nf) * 2.0 ** 20) / 2.0 ** 20
    return t, y, W, f


def check_against_long_double():
    """The PyTorch route on the CPU against tests/_bls_ref.py: bls_ref_ld on the tests' base case."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _bls_ref import base_case, bls_ref_ld
    t, f, y = base_case()
    W = 0.5 + np.random.default_rng(1).random(len(t))
    for nbins, k0, k1 in ((64, 1, 8), (100, 2, 12)):
        r = bls_ref_ld(y, t, f, W, nbins, k0, k1)
        p, b, k = torch_bls(torch, torch.tensor(y), torch.tensor(t), torch.tensor(W), f, nbins, k0, k1, 16)
        assert np.array_equal(b.numpy(), r["start"][:, 0]) and np.array_equal(k.numpy(), r["width"][:, 0]), "the PyTorch route finds other boxes than the reference"
        assert np.max(np.abs(p.numpy() - r["power"][:, 0].astype(np.float64))) <= 1e-12, "the PyTorch route's power is off the reference"


def child(N, Nf, nbins, reps, dense_limit):
    import torch
    import lpvspectral_jl_amd as L
    t, y, W, f = record(N, Nf)
    kmin, kmax = widths(nbins)
    yd, td, Wd = (torch.tensor(a, device="cuda") for a in (y, t, W))
    sub = int(max(1, min(Nf, dense_limit // N)))
    chunk = int(max(1, min(sub, (1 << 25) // N)))                             # (chunk, N) doubles: at most 256 MiB each

    def new():
        R = L.bls(yd, td, f, W=Wd, nbins=nbins, q=Q)
        return R, L.bls_last_timing()

    def old():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        p, b, k = torch_bls(torch, yd, td, Wd, f[:sub], nbins, kmin, kmax, chunk)
        e1.record()
        torch.cuda.synchronize()
        return p.cpu().numpy(), b.cpu().numpy(), k.cpu().numpy(), e0.elapsed_time(e1)

    R, tm = new()
    p, b, k, _ = old()
    assert np.max(np.abs(R.power[:sub] - p)) <= 1e-9, "the two routes disagree"
    agree = float(np.mean((R.start[:sub] == b) & (R.width[:sub] == k)))
    nt, ns_, nq, nsc, ot = [], [], [], [], []
    for _ in range(reps):
        _, tm = new()
        nt.append(tm["total_ms"]); ns_.append(tm["search_ms"]); nq.append(tm["quantise_ms"]); nsc.append(tm["scan_ms"])
        ot.append(old()[3] * Nf / sub)
    med = lambda v: float(np.median(v))       # noqa: E731
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "Nf": Nf, "nbins": nbins, "kmin": kmin, "kmax": kmax, "F": tm["F"], "lds": tm["lds_bytes"],
                      "boxes": tm["boxes"], "sub": sub, "agree": agree, "peak": float(f[int(np.argmax(R.power))]), "new_total": med(nt), "new_search": med(ns_),
                      "new_quant": med(nq), "new_scan": med(nsc), "old_total": med(ot)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds a configuration's child process may take")
    ap.add_argument("--dense-limit", type=int, default=1 << 31, help="elements Nf N beyond which the torch route runs on a part of the frequencies")
    ap.add_argument("--samples", type=int, nargs="*", default=[1 << 12, 1 << 16, 1 << 18])
    ap.add_argument("--freqs", type=int, nargs="*", default=[4096, 65536])
    ap.add_argument("--bins", type=int, nargs="*", default=[128, 512])
    ap.add_argument("--child", type=int, nargs=3, default=None, metavar=("N", "Nf", "nbins"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.child[2], a.reps, a.dense_limit)
        return 0
    check_against_long_double()
    configs = [(N, Nf, nb) for N in a.samples for Nf in a.freqs for nb in a.bins]

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):                                                               # (the file grows line by line: a run that is cut short leaves what it had)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    head = False
    for N, Nf, nb in configs:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--dense-limit", str(a.dense_limit), "--child", str(N), str(Nf),
                                  str(nb)], timeout=a.limit, check=True, stdout=subprocess.PIPE, text=True).stdout
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            emit(f"# N = {N}, Nf = {Nf}, nbins = {nb}: the child process failed ({type(e).__name__}); stopped here")
            return 1
        r = json.loads(out.strip().split("\n")[-1])
        if not head:
            emit("# bls against a chunked PyTorch evaluation of the same definition (fold, scatter_add_ into float64 histograms, cumsum, every box, arg-max),")
            emit(f"# {r['device']}, one signal with weights, device-resident y, t, W; f over [0.05, 0.5] (mean spacing of t: 1), q = (0.01, 0.1), dips only;")
            emit(f"# ms, median of {a.reps} after a warm-up; new: HIP events of the library, torch: torch.cuda events, scaled by Nf / sub where sub < Nf;")
            emit("# the PyTorch route was held to the long-double reference of the tests on the CPU before the first row; `same box`: share of the frequencies")
            emit("# (of the first sub) where both routes return the same box (the powers agree to 1e-9 everywhere)")
            emit(f"{'N':>7} {'Nf':>6} {'nbins':>5} {'widths':>7} {'F':>2} {'LDS':>6} | {'new total':>9} {'scan':>7} {'quant':>7} {'search':>9} {'ns/pair':>8} {'ns/box':>7} | "
                 f"{'torch':>11} {'sub':>6} {'same box':>8} | {'torch/new':>9}")
            head = True
        per = r["new_search"] * 1e6 / (float(N) * Nf)
        box = r["new_search"] * 1e6 / r["boxes"]
        emit(f"{N:>7} {Nf:>6} {nb:>5} {str(r['kmin']) + '..' + str(r['kmax']):>7} {r['F']:>2} {r['lds']:>6} | {r['new_total']:>9.3f} {r['new_scan']:>7.3f} "
             f"{r['new_quant']:>7.3f} {r['new_search']:>9.3f} {per:>8.4f} {box:>7.3f} | {r['old_total']:>11.3f} {r['sub']:>6} {r['agree']:>8.4f} | "
             f"{r['old_total'] / r['new_total']:>9.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
