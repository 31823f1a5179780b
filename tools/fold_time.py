"""Time of pdm and conditional_entropy (csrc/fold.hip) against the routes a user had before they existed.

  pdm:  bls(..., return_hist=True) at nbins = nfine with a single width (the only way to the folded integer histograms), its histograms
        copied to the host, and the pooled between-bin sum in numpy.  `bls` is the HIP-event time of that call (histogram copy included),
        `numpy` the host time of the epilogue (time.perf_counter).
  cent: a chunked PyTorch evaluation of the same definition on the device -- fold, torch.bincount over (frequency, phase bin, value bin),
        the entropy in torch -- timed by torch.cuda events.  Where Nf N is more than --dense-limit elements it runs on the first `sub`
        frequencies only and the time is scaled by Nf / sub (its chunks are independent and equal).
Neither baseline is the code under test.  Before anything is timed both are held to tests/_fold_ref.py on the CPU.

One record of N non-uniform times (multiples of 2^-10, mean spacing 1, in random order), weights in [0.5, 2] (pdm), one signal: noise of
sigma 1/4 under a unit sawtooth at f = 0.1171875; Nf frequencies over [0.05, 0.5], multiples of 2^-20: every product f t is exact, so all
routes fold every sample into the same bin and have to agree (asserted per configuration, to 1e-9).  Device-resident y, t and W.  Every
(N, Nf) runs in a child process of its own under its own time limit; the tool stops at the first child that fails.  Per configuration one
warm-up of each route, then --reps repetitions; reported is the median.  `ns/pair`: the fold phase (fold and epilogue kernels) per
(sample, frequency), in nanoseconds.  The conditional entropy at (10, 5) is also run with LPVS_CENT_COPIES = 1, 2 and 4: whether private
copies of the count histogram pay at few cells is measured here, not assumed.

    timeout -k 10 1100 python tools/fold_time.py [--out profiles/fold_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

os.environ.setdefault("LPVS_EXPERIMENTS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PDM = ((10, 1), (5, 2), (128, 1))
CENT = ((10, 5, 0), (10, 5, 1), (10, 5, 2), (10, 5, 4), (64, 16, 0))           # (nbins, mbins, the copies knob; 0: the plan's rule)


def numpy_pdm(hist, covers, shift_y, shift_w, YY):
    """explained per frequency from bls's raw histograms of ONE signal: hist (Nf, 2, nfine) int64, row 0 the weights, row 1 the signal."""
    def coarse(H):
        P = np.concatenate([np.zeros((len(H), 1), H.dtype), np.cumsum(np.concatenate([H, H], axis=1), axis=1)], axis=1)
        return P[:, covers:covers + H.shape[1]] - P[:, :H.shape[1]]
    r, s = coarse(hist[:, 0]).astype(np.float64), coarse(hist[:, 1]).astype(np.float64)
    R, S = hist[:, 0].sum(axis=1).astype(np.float64), hist[:, 1].sum(axis=1).astype(np.float64)
    has = r > 0
    sb = np.where(has, s * s / np.where(has, r, 1.0), 0.0).sum(axis=1) / covers - S * S / R
    return np.minimum(1.0, np.ldexp(np.maximum(sb, 0.0), shift_w - 2 * shift_y) / YY), has.sum(axis=1)


def torch_cent(torch, y, t, f, nbins, mbins, chunk):
    """-> the entropy per frequency; everything on the device of y."""
    N, cells = len(t), nbins * mbins
    ymin, ymax = y.min(), y.max()
    j = torch.clamp(torch.floor((y - ymin) / (ymax - ymin) * mbins).long(), max=mbins - 1)
    out = []
    for k0 in range(0, len(f), chunk):
        fd = torch.as_tensor(f[k0:k0 + chunk], device=y.device)
        ph = fd[:, None] * t[None, :]
        ph = ph - torch.floor(ph)
        i = torch.clamp((ph * nbins).long(), max=nbins - 1)
        idx = torch.arange(len(fd), device=y.device)[:, None] * cells + i * mbins + j[None, :]
        cnt = torch.bincount(idx.reshape(-1), minlength=len(fd) * cells).reshape(len(fd), nbins, mbins).double()
        ni = cnt.sum(dim=2, keepdim=True).expand_as(cnt)
        has = cnt > 0
        one = torch.ones_like(cnt)
        out.append((cnt * torch.log(torch.where(has, ni, one) / torch.where(has, cnt, one))).sum(dim=(1, 2)) / N)
    return torch.cat(out)


def record(N, Nf):
    rng = np.random.default_rng(N)
    t = rng.permutation(np.round((np.arange(N) + rng.random(N)) * 1024) / 1024)
    y = np.mod(0.1171875 * t, 1.0) + 0.25 * rng.standard_normal(N)
    W = rng.uniform(0.5, 2.0, N)
    f = np.round(np.linspace(0.05, 0.5, Nf) * 2.0 ** 20) / 2.0 ** 20
    return t, y, W, f


def check_baselines_on_the_cpu():
    """The two baselines against the models of tests/_fold_ref.py on the tests' planted case."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _fold_ref import cent_model, pdm_model, sawtooth_case
    t, f, y = sawtooth_case()
    W = 0.5 + np.random.default_rng(1).random(len(t))
    for nbins, covers in PDM:
        m = pdm_model(y, t, f, W, nbins, covers, True)
        w = W / W.sum()
        YY = float((w * (y - (w * y).sum()) ** 2).sum())
        e, M = numpy_pdm(m["hist"], covers, m["shy"][0], 60, YY)
        assert np.array_equal(M, m["nonempty"]) and np.max(np.abs(e - m["explained"][:, 0])) <= 1e-12, "the numpy epilogue is off the model"
    for nbins, mbins in ((10, 5), (64, 16)):
        H = torch_cent(torch, torch.tensor(y), torch.tensor(t), f, nbins, mbins, 16).numpy()
        assert np.max(np.abs(H - cent_model(y, t, f, nbins, mbins)["entropy"][:, 0])) <= 1e-12, "the PyTorch route is off the model"


def child(N, Nf, reps, dense_limit):
    import torch
    import lpvspectral_jl_amd as L
    t, y, W, f = record(N, Nf)
    yd, td, Wd = (torch.tensor(a, device="cuda") for a in (y, t, W))
    w = W / W.sum()
    YY = float((w * (y - (w * y).sum()) ** 2).sum())
    med = lambda v: float(np.median(v))       # noqa: E731
    rows = []
    for nbins, covers in PDM:
        nfine = nbins * covers

        def new():
            R = L.pdm(yd, td, f, W=Wd, nbins=nbins, covers=covers)
            return R, L.pdm_last_timing()

        def old():
            B = L.bls(yd, td, f, W=Wd, nbins=nfine, q=(0.5 / nfine, 0.5 / nfine), return_hist=True)
            tm = L.bls_last_timing()
            h0 = time.perf_counter()
            e, M = numpy_pdm(B.hist, covers, tm["shift_y_min"], tm["shift_w"], YY)
            return e, M, tm["total_ms"], (time.perf_counter() - h0) * 1e3

        R, tm = new()
        e, M, _, _ = old()
        assert np.array_equal(M, R.nonempty) and np.max(np.abs(R.explained - e)) <= 1e-9, "the two routes disagree"
        a = {k: [] for k in ("total_ms", "scan_ms", "prepare_ms", "fold_ms")}
        od, oh = [], []
        for _ in range(reps):
            _, tm = new()
            for k in a:
                a[k].append(tm[k])
            _, _, d, h = old()
            od.append(d); oh.append(h)
        rows.append(dict(kind="pdm", bins=f"{nbins}x{covers}", F=tm["F"], ts=tm["ts"], copies=tm["copies"], lds=tm["lds_bytes"], sub=Nf, base_dev=med(od),
                         base_host=med(oh), peak=float(f[int(np.argmax(R.explained))]), **{k: med(v) for k, v in a.items()}))
    sub = int(max(1, min(Nf, dense_limit // N)))
    chunk = int(max(1, min(sub, (1 << 24) // N)))                             # (chunk, N) doubles and int64s: at most 128 MiB each
    for nbins, mbins, knob in CENT:
        def new():
            if knob:
                os.environ["LPVS_CENT_COPIES"] = str(knob)
            try:
                R = L.conditional_entropy(yd, td, f, nbins=nbins, mbins=mbins)
            finally:
                os.environ.pop("LPVS_CENT_COPIES", None)
            return R, L.cent_last_timing()

        def old():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            H = torch_cent(torch, yd, td, f[:sub], nbins, mbins, chunk)
            e1.record()
            torch.cuda.synchronize()
            return H.cpu().numpy(), e0.elapsed_time(e1)

        R, tm = new()
        assert np.max(np.abs(R.entropy[:sub] - old()[0])) <= 1e-9, "the two routes disagree"
        a = {k: [] for k in ("total_ms", "scan_ms", "prepare_ms", "fold_ms")}
        od = []
        for _ in range(reps):
            _, tm = new()
            for k in a:
                a[k].append(tm[k])
            od.append(old()[1] * Nf / sub if not knob else 0.0)
        rows.append(dict(kind="cent", bins=f"{nbins}x{mbins}", F=tm["F"], ts=tm["ts"], copies=tm["copies"], lds=tm["lds_bytes"], sub=sub, base_dev=med(od), base_host=0.0,
                         peak=float(f[int(np.argmin(R.entropy))]), knob=knob, **{k: med(v) for k, v in a.items()}))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "Nf": Nf, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=170, help="seconds the child process of one (N, Nf) may take")
    ap.add_argument("--dense-limit", type=int, default=1 << 28, help="elements Nf N beyond which the torch route runs on a part of the frequencies")
    ap.add_argument("--samples", type=int, nargs="*", default=[1 << 12, 1 << 16, 1 << 18])
    ap.add_argument("--freqs", type=int, nargs="*", default=[4096, 65536])
    ap.add_argument("--child", type=int, nargs=2, default=None, metavar=("N", "Nf"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.dense_limit)
        return 0
    check_baselines_on_the_cpu()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):                                                               # (the file grows line by line: a run that is cut short leaves what it had)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    head = False
    for N in a.samples:
        for Nf in a.freqs:
            try:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--dense-limit", str(a.dense_limit), "--child", str(N), str(Nf)],
                                     timeout=a.limit, check=True, stdout=subprocess.PIPE, text=True).stdout
            except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
                emit(f"# N = {N}, Nf = {Nf}: the child process failed ({type(e).__name__}); stopped here")
                return 1
            r = json.loads(out.strip().split("\n")[-1])
            if not head:
                emit("# pdm against bls(return_hist=True) at nbins = nfine plus a numpy epilogue (bls: HIP events of that call, numpy: host time of the epilogue);")
                emit("# conditional_entropy against a chunked PyTorch fold + bincount + entropy on the device (torch.cuda events, scaled by Nf / sub where sub < Nf);")
                emit(f"# {r['device']}, one signal (pdm: with weights), device-resident y, t, W; f over [0.05, 0.5] (mean spacing of t: 1);")
                emit(f"# ms, median of {a.reps} after a warm-up; new: HIP events of the library; both baselines were held to the tests' models on the CPU before the first")
                emit("# row and agree with the new call to 1e-9 in every row; knob: LPVS_CENT_COPIES (-: the plan's rule; baseline not repeated for forced copies)")
                emit(f"{'kind':>4} {'N':>7} {'Nf':>6} {'bins':>6} {'F':>2} {'TS':>2} {'cp':>2} {'knob':>4} {'LDS':>6} | {'new total':>9} {'scan':>7} {'prep':>7} {'fold':>9} {'ns/pair':>8} | "
                     f"{'base dev':>10} {'base host':>9} {'sub':>6} | {'base/new':>8}")
                head = True
            for q in r["rows"]:
                per = q["fold_ms"] * 1e6 / (float(N) * Nf)
                base = q["base_dev"] + q["base_host"]
                knob = str(q.get("knob") or "-")
                emit(f"{q['kind']:>4} {N:>7} {Nf:>6} {q['bins']:>6} {q['F']:>2} {q['ts']:>2} {q['copies']:>2} {knob:>4} {q['lds']:>6} | {q['total_ms']:>9.3f} {q['scan_ms']:>7.3f} "
                     f"{q['prepare_ms']:>7.3f} {q['fold_ms']:>9.3f} {per:>8.4f} | {q['base_dev']:>10.3f} {q['base_host']:>9.3f} {q['sub']:>6} | "
                     + (f"{base / q['total_ms']:>8.1f}" if base > 0 else f"{'':>8}"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
