"""Time of wwz (csrc/wwz.hip) against the route a user had before it existed: a chunked PyTorch evaluation of the same sums on the device
-- dense (tau chunk) x Nf x N weights W exp(-a (t - tau)^2) cut at the radius, batched matmuls against the tables of cos, sin, cos 2, sin 2,
y cos, y sin (Nf x N, formed once per call) -- and the closed-form floating-mean fit in torch.

One record of N sorted non-uniform times of mean spacing 1, weights in [0.5, 2], one signal; Nf frequencies spanning the decade
[0.025, 0.25], linear or logarithmic; Ntau equally spaced times over the record; c = 1 / (8 pi^2), wmin = 1e-9 (a cell reaches 6.44
periods: 26 to 258 samples either side).  Device-resident y, t and W on both routes.  Every configuration runs in a child process of its
own under its own time limit; the tool stops at the first child that fails.  Per configuration one warm-up of each route (the two must
agree to 1e-9 in power and Neff on the times both computed), then --reps repetitions; reported is the median.
  new:   the HIP-event times of wwz_last_timing: the whole call (`total`), the sums kernel (`sums`), the ranges with the work list
         (`ranges`: two launches, the copy of the edges to the host and the host's layout of the items) and the epilogue (`epi`).
  torch: torch.cuda events around the whole evaluation.  The dense route costs Ntau Nf N whatever the radius; where that is more than
         --dense-limit elements it is run on the first `sub` times only and the time is scaled by Ntau / sub (its chunks are independent
         and equal, so the scaling is exact up to the tables formed once, which are counted in full): the column `sub` says so.
The model of the new call per useful (sample, frequency, time) triple -- one inside its cell: one exp and about 14 fused multiply-adds, and a
quarter of a sincospi at TT = 4 -- is set against the 2.4e-9 ms per sincospi of DESIGN.md 4.12 in the column `ns/triple` (sums kernel
time per USEFUL triple, in nanoseconds); `staged/useful` is the work-list's count of triples the kernel stages against those.

    timeout -k 10 1100 python tools/wwz_time.py [--out profiles/wwz_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_wwz(torch, y, t, W, f, tau, c, radius, chunk):
    """-> power, neff (Nf, len(tau)) by dense weights; everything on the device of y."""
    two_pi = 2 * np.pi
    fd, rd = (torch.as_tensor(v, device=y.device) for v in (f, radius))
    a = c * (two_pi * fd) ** 2
    turns = fd[:, None] * t[None, :]
    ph = two_pi * (turns - torch.round(turns))
    cs, sn = torch.cos(ph), torch.sin(ph)
    yc = y - (W * y).sum() / W.sum()
    X = torch.stack([cs, sn, cs * cs - sn * sn, 2 * sn * cs, cs * yc[None, :], sn * yc[None, :]], dim=2)      # (Nf, N, 6)
    V = torch.stack([torch.ones_like(yc), yc, yc * yc], dim=1)                                               # (N, 3)
    power, neff = [], []
    for j0 in range(0, len(tau), chunk):
        tj = torch.as_tensor(tau[j0:j0 + chunk], device=y.device)
        d = t[None, None, :] - tj[None, :, None]                                                             # (1, chunk, N)
        G = W[None, None, :] * torch.exp(-a[:, None, None] * d * d) * (d.abs() <= rd[:, None, None])          # (Nf, chunk, N)
        S6 = torch.bmm(G, X)                                                                                 # (Nf, chunk, 6)
        S3 = G @ V                                                                                           # (Nf, chunk, 3)
        sw2 = (G * G).sum(dim=2)
        sw = S3[..., 0]
        live = sw > 0
        den = torch.where(live, sw, torch.ones_like(sw))
        C, S, C2, S2, YC, YS = (S6[..., i] / den for i in range(6))
        Y, YY = S3[..., 1] / den, S3[..., 2] / den
        CC, SS, CS = 0.5 * (1 + C2) - C * C, 0.5 * (1 - C2) - S * S, 0.5 * S2 - C * S
        YYm, YCm, YSm = YY - Y * Y, YC - Y * C, YS - Y * S
        D = CC * SS - CS * CS
        ok = live & (D > 2.0 ** -40)
        Ds = torch.where(ok, D, torch.ones_like(D))
        p = (SS * YCm * YCm + CC * YSm * YSm - 2 * CS * YCm * YSm) / Ds
        power.append(torch.where(ok & (YYm > 0), p / torch.where(YYm > 0, YYm, torch.ones_like(YYm)), torch.zeros_like(p)))
        neff.append(torch.where(live, sw * sw / torch.where(live, sw2, torch.ones_like(sw2)), torch.zeros_like(sw)))
    return torch.cat(power, dim=1), torch.cat(neff, dim=1)


def child(N, Nf, Ntau, log, reps, dense_limit):
    import torch
    import lpvspectral_jl_amd as L
    rng = np.random.default_rng(N)
    t = np.sort(rng.random(N)) * N
    y = np.cos(2 * np.pi * 0.05 * t) + 0.4 * np.cos(2 * np.pi * 0.2 * t) * (t > N / 2) + rng.standard_normal(N)
    W = rng.uniform(0.5, 2.0, N)
    f = np.geomspace(0.025, 0.25, Nf) if log else np.linspace(0.025, 0.25, Nf)
    tau = np.linspace(t[0], t[-1], Ntau)
    c = 1.0 / (8.0 * np.pi ** 2)
    radius = L.wwz_radius(f, c, 1e-9)
    yd, td, Wd = (torch.tensor(a, device="cuda") for a in (y, t, W))
    sub = int(max(1, min(Ntau, dense_limit // (Nf * N))))
    chunk = int(max(1, min(sub, (1 << 28) // (Nf * N))))                      # the dense weights of a chunk: at most 2 GiB

    def new():
        R = L.wwz(yd, td, f, tau=tau, c=c, wmin=1e-9, W=Wd)
        return R, L.wwz_last_timing()

    def old():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        P, ne = torch_wwz(torch, yd, td, Wd, f, tau[:sub], c, radius, chunk)
        e1.record()
        torch.cuda.synchronize()
        return P.cpu().numpy(), ne.cpu().numpy(), e0.elapsed_time(e1)

    R, tm = new()
    P, ne, _ = old()
    assert np.max(np.abs(R.power[:, :sub] - P)) <= 1e-9 and np.max(np.abs(R.neff[:, :sub] - ne)) <= 1e-9 * np.max(ne), "the two routes disagree"
    nt, nsums, nrng, nepi, ot = [], [], [], [], []
    for _ in range(reps):
        _, tm = new()
        nt.append(tm["total_ms"]); nsums.append(tm["sums_ms"]); nrng.append(tm["ranges_ms"]); nepi.append(tm["epilogue_ms"])
        ot.append(old()[2] * Ntau / sub)
    med = lambda v: float(np.median(v))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "Nf": Nf, "Ntau": Ntau, "grid": "log" if log else "lin", "tt": tm["tt"], "items": tm["items"],
                      "slab": tm["slab"], "empty": tm["empty"], "staged": tm["staged"], "useful": tm["useful"], "sub": sub, "new_total": med(nt), "new_sums": med(nsums),
                      "new_ranges": med(nrng), "new_epi": med(nepi), "old_total": med(ot)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a configuration's child process may take")
    ap.add_argument("--dense-limit", type=int, default=1 << 31, help="elements Ntau Nf N beyond which the torch route runs on a part of the times")
    ap.add_argument("--samples", type=int, nargs="*", default=[1 << 14, 1 << 17, 1 << 20])
    ap.add_argument("--freqs", type=int, nargs="*", default=[128, 512])
    ap.add_argument("--times", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--child", type=int, nargs=4, default=None, metavar=("N", "Nf", "Ntau", "log"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.child[2], bool(a.child[3]), a.reps, a.dense_limit)
        return 0
    configs = [(N, Nf, Ntau, log) for N in a.samples for Nf in a.freqs for Ntau in a.times for log in (0, 1)]

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):                                                               # (the file grows line by line: a run that is cut short leaves what it had)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    head = False
    for N, Nf, Ntau, log in configs:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--dense-limit", str(a.dense_limit), "--child", str(N), str(Nf),
                                  str(Ntau), str(log)], timeout=a.limit, check=True, stdout=subprocess.PIPE, text=True).stdout
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            emit(f"# N = {N}, Nf = {Nf}, Ntau = {Ntau}, log = {log}: the child process failed ({type(e).__name__}); stopped here")
            return 1
        r = json.loads(out.strip().split("\n")[-1])
        if not head:
            emit("# wwz against a chunked PyTorch evaluation of the same sums with dense (tau chunk) x Nf x N weights, batched matmuls and the closed-form fit,")
            emit(f"# {r['device']}, one signal, device-resident y, t, W; f over [0.025, 0.25] (mean spacing of t: 1), c = 1/(8 pi^2), wmin = 1e-9;")
            emit(f"# ms, median of {a.reps} after a warm-up; new: HIP events of the library, torch: torch.cuda events, scaled by Ntau / sub where sub < Ntau")
            emit(f"{'N':>8} {'Nf':>4} {'Ntau':>5} {'grid':>4} {'TT':>2} {'items':>6} {'slab':>6} {'empty':>6} {'staged/useful':>13} | {'new total':>9} {'ranges':>7} {'sums':>8} "
                 f"{'epi':>6} {'ns/triple':>9} | {'torch':>12} {'sub':>5} | {'torch/new':>10}")
            head = True
        ratio = r["staged"] / r["useful"] if r["useful"] else float("nan")
        per = r["new_sums"] * 1e6 / r["useful"] if r["useful"] else float("nan")
        emit(f"{N:>8} {Nf:>4} {Ntau:>5} {r['grid']:>4} {r['tt']:>2} {r['items']:>6} {r['slab']:>6} {r['empty']:>6} {ratio:>13.2f} | {r['new_total']:>9.3f} "
             f"{r['new_ranges']:>7.3f} {r['new_sums']:>8.3f} {r['new_epi']:>6.3f} {per:>9.4f} | {r['old_total']:>12.3f} {r['sub']:>5} | {r['old_total'] / r['new_total']:>10.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
