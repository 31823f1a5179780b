"""Time of clean (csrc/clean.hip) against the route a user had before it existed: lombscargle(..., return_sums=True) on the 2 Nf - 1
frequencies m df for the sums C, S, YC, YS, then the CLEAN loop in PyTorch on the same device -- per iteration an argmax over the
admissible bins (with its read-back to the host), the scalar step and two sliced complex updates of the residual.

  new:   L.clean(...) with device-resident y and t; the library's HIP events: the sums, the loop, the restoration and the total.
  base:  `sums` the HIP-event total of the lombscargle call, `loop` torch.cuda events around the PyTorch loop.  The loop handles one signal at
         a time (the slices differ per signal); with ns > --base-signals it runs on the first few signals and is scaled by ns over that
         number (the signals are independent and alike).
The baseline is not the code under test: before anything is timed it is held to the float64 model of tests/_clean_ref.py on the CPU (20
iterations of the planted case, 1e-12), and in every configuration its components after the run agree with the new call's to 1e-9.

One record of N = 2^16 non-uniform times (multiples of 2^-10, mean spacing 1, sorted), df = 2^-18 = 1 / (4 N), unit weights, signals of
three lines and noise; every product (m df) t is exact.  Every configuration runs in a child process of its own under its own time limit
(ns = 64 is ONE process); the tool stops at the first child that fails.  At Nf = 4096 the loop is also run with LPVS_CLEAN_RESIDUAL=global:
the residency in LDS is kept only if it is not slower.  Per configuration one warm-up of each route, then --reps repetitions; the median.

    timeout -k 10 1100 python tools/clean_time.py [--out profiles/clean_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

os.environ.setdefault("LPVS_EXPERIMENTS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1 << 16
DF = 2.0 ** -18
GAIN = 0.5
# (Nf, ns, the residual knob)
CONFIGS = ((4096, 1, ""), (4096, 1, "global"), (4096, 64, ""), (4096, 64, "global"), (65536, 1, ""), (65536, 64, ""))


def torch_loop(torch, D, Wn, gain, niter):
    """The CLEAN loop of include/lpvspectral.h g11 for ONE signal as a user writes it in PyTorch: D (Nf,), Wn (2 Nf - 1,) complex128 on one
    device -> (R, C)."""
    Nf = D.shape[0]
    K = Nf - 1
    full = torch.cat([torch.conj(torch.flip(Wn[1:], dims=[0])), Wn])         # full[j] = Wn_{j - 2K}
    w2 = Wn[0:2 * K + 1:2]
    den = 1.0 - (w2.real * w2.real + w2.imag * w2.imag)
    adm = den >= 2.0 ** -20
    R, Cc = D.clone(), torch.zeros_like(D)
    for _ in range(niter):
        P = torch.where(adm, R.real * R.real + R.imag * R.imag, -1.0)
        p = int(torch.argmax(P))                                              # the read-back of every iteration
        a = (R[p] - torch.conj(R[p]) * w2[p]) / den[p]
        c = gain * a
        Cc[p] += c
        R -= c * full[2 * K - p:2 * K - p + Nf]
        R -= torch.conj(c) * Wn[p:p + Nf]
    return R, Cc


def check_baseline_on_the_cpu():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _clean_ref as ref
    case = ref.loop_case("planted")
    D, Wn = ref.host_spectra(case)
    m = ref.clean_model(D[0], Wn, 0.5, 20, 0.0)
    R, Cc = torch_loop(torch, torch.tensor(D[0]), torch.tensor(Wn), 0.5, 20)
    assert np.max(np.abs(Cc.numpy() - ref.to_complex(*m["C"]))) <= 1e-12 and np.max(np.abs(R.numpy() - ref.to_complex(*m["R"]))) <= 1e-12, \
        "the PyTorch loop is off the model"


def record(ns):
    rng = np.random.default_rng(ns)
    t = np.sort(np.round((np.arange(N) + rng.random(N)) * 1024) / 1024)
    c = np.arange(ns)[None, :]
    y = (np.cos(2 * np.pi * (1000 * DF) * t[:, None] + 0.3 * c) + 0.6 * np.cos(2 * np.pi * (2500 * DF) * t[:, None] - 1.1)
         + 0.3 * np.cos(2 * np.pi * (3900 * DF) * t[:, None] + 0.1 * c) + 0.5 * rng.standard_normal((N, ns)))
    return t, y


def child(Nf, ns, knob, niter, reps, base_signals):
    import torch
    import lpvspectral_jl_amd as L
    t, y = record(ns)
    yd, td = torch.tensor(y, device="cuda"), torch.tensor(t, device="cuda")
    f = np.arange(2 * Nf - 1) * DF
    med = lambda v: float(np.median(v))       # noqa: E731
    sub = min(ns, base_signals)

    def new():
        if knob:
            os.environ["LPVS_CLEAN_RESIDUAL"] = knob
        try:
            r = L.clean(yd, td, df=DF, Nf=Nf, gain=GAIN, niter=niter, center_time=False)
        finally:
            os.environ.pop("LPVS_CLEAN_RESIDUAL", None)
        return r, L.clean_last_timing()

    def old():
        _, s = L.lombscargle(yd, td, f, return_sums=True)
        sums_ms = L.lombscargle_last_timing()["total_ms"]
        Wn = torch.tensor(s["C"] - 1j * s["S"], device="cuda")
        D = torch.tensor(s["YC"][:sub, :Nf] - 1j * s["YS"][:sub, :Nf], device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = [torch_loop(torch, D[c], Wn, GAIN, niter) for c in range(sub)]
        e1.record()
        torch.cuda.synchronize()
        return torch.stack([o[1] for o in out]).cpu().numpy(), sums_ms, e0.elapsed_time(e1) * ns / sub

    r, tm = new()
    Cb, _, _ = old()
    assert tm["iterations_min"] == niter, "the new call stopped early"
    agree = float(np.max(np.abs(np.atleast_2d(r.components.T)[:sub] - Cb)))
    assert agree <= 1e-9, f"the two routes disagree: {agree}"
    a = {k: [] for k in ("total_ms", "moments_ms", "sums_ms", "loop_ms", "restore_ms", "copy_ms")}
    bs, bl = [], []
    for _ in range(reps):
        _, tm = new()
        for k in a:
            a[k].append(tm[k])
        _, s_ms, l_ms = old()
        bs.append(s_ms); bl.append(l_ms)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), Nf=Nf, ns=ns, knob=knob, niter=niter, residual=tm["residual"], threads=tm["threads"],
                          lds=tm["lds_bytes"], path=tm["path"], admissible=tm["admissible"], sub=sub, base_sums=med(bs), base_loop=med(bl), agree=agree,
                          **{k: med(v) for k, v in a.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--niter", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=170, help="seconds the child process of one configuration may take")
    ap.add_argument("--base-signals", type=int, default=2, help="signals the PyTorch loop runs on (scaled by ns over that number)")
    ap.add_argument("--child", nargs=3, default=None, metavar=("Nf", "ns", "knob"))
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.child[2] if a.child[2] != "-" else "", a.niter, a.reps, a.base_signals)
        return 0
    check_baseline_on_the_cpu()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(s):                                                               # (the file grows line by line: a run that is cut short leaves what it had)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    head = False
    for Nf, ns, knob in CONFIGS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--niter", str(a.niter), "--base-signals", str(a.base_signals),
                                  "--child", str(Nf), str(ns), knob or "-"], timeout=a.limit, check=True, stdout=subprocess.PIPE, text=True).stdout
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            emit(f"# Nf = {Nf}, ns = {ns}, knob = {knob or '-'}: the child process failed ({type(e).__name__}); stopped here")
            return 1
        q = json.loads(out.strip().split("\n")[-1])
        if not head:
            emit("# clean (one call: sums, loop, restoration) against lombscargle(return_sums=True) on the 2 Nf - 1 frequencies plus the CLEAN loop in PyTorch")
            emit("# on the same device (argmax with its read-back, the scalar step, two sliced complex updates per iteration; one signal at a time, run on `sub`")
            emit(f"# signals and scaled by ns / sub); {q['device']}, N = {N}, df = 2^-18, gain {GAIN}, {a.niter} iterations, unit weights, device-resident y and t;")
            emit(f"# ms, median of {a.reps} after a warm-up; new: HIP events of the library; base sums: HIP events of lombscargle, base loop: torch.cuda events;")
            emit("# the PyTorch loop was held to the tests' model on the CPU before the first row and agrees with the new call's components to 1e-9 in every row;")
            emit("# knob: LPVS_CLEAN_RESIDUAL (-: the plan's rule); us/it: the loop per iteration")
            emit(f"{'Nf':>6} {'ns':>3} {'knob':>6} {'resid':>6} {'thr':>4} {'LDS':>6} {'path':>6} | {'new total':>9} {'moments':>8} {'sums':>8} {'loop':>9} {'us/it':>7} {'restore':>8} {'copy':>7} | "
                 f"{'base sums':>9} {'base loop':>10} {'us/it':>8} {'sub':>3} | {'base/new':>8} {'loops':>7}")
            head = True
        new_part, base = q["total_ms"], q["base_sums"] + q["base_loop"]
        emit(f"{Nf:>6} {ns:>3} {(knob or '-'):>6} {q['residual']:>6} {q['threads']:>4} {q['lds']:>6} {q['path']:>6} | {q['total_ms']:>9.3f} {q['moments_ms']:>8.3f} {q['sums_ms']:>8.3f} "
             f"{q['loop_ms']:>9.3f} {q['loop_ms'] * 1e3 / a.niter:>7.2f} {q['restore_ms']:>8.3f} {q['copy_ms']:>7.3f} | {q['base_sums']:>9.3f} {q['base_loop']:>10.3f} "
             f"{q['base_loop'] * 1e3 / a.niter:>8.1f} {q['sub']:>3} | {base / new_part:>8.1f} {q['base_loop'] / q['loop_ms']:>7.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
