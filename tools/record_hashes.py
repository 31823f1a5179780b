#!/usr/bin/env python3
"""One line per call of the transforms of uneven records (csrc/uneven.hip: lombscargle and its several-harmonic, windowed and bootstrap
forms, time_windows, wwz, bls): a SHA-256 of every returned array and every slot of the call's *_last_timing that is not a time.  The
cases are the smallest that reach each path of the host drivers -- N = 600 is three blocks of the scan, the last one partial -- once with
host arrays and once with device tensors for t, y and W, and two calls through ctypes with device-resident outputs.  Two builds of the
library compute the same thing exactly when their outputs are identical:

    LPVS_LIBRARY=/path/to/other/liblpvspectral.so tools/record_hashes.py > a.txt;  tools/record_hashes.py > b.txt;  cmp a.txt b.txt

Inputs are fixed (seeded); nothing in the output depends on time.  profiles/record_hashes.txt is the output on an MI355X."""
import ctypes as C
import hashlib
import os
import sys

os.environ.setdefault("LPVS_EXPERIMENTS", "1")                                # LPVS_LOMB_BLOCK and LPVS_LOMB_BOOT_MB are experiment knobs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import lpvspectral_jl_amd as L
from lpvspectral_jl_amd import _lib
from test_gpu_pool_fill import _flat, _is_time, _lomb_record, _irregular

N = 600
D = 1.0 / 64.0


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def report(name, result, timing):
    """`result`: whatever the call returned (flattened as tests/test_gpu_pool_fill.py flattens it); `timing`: the *_last_timing dict."""
    arrays = " ".join(f"{k or '.'}:{sha(v)}" for k, v in sorted(_flat(result).items()))
    plan = " ".join(f"{k}={v}" for k, v in sorted(timing.items()) if not _is_time(k))
    print(f"{name:44s} {arrays} | {plan}", flush=True)


def record(ns, N=N):
    t, y, W = _lomb_record(N, ns)
    return t, (y if ns > 1 else y[:, 0]), W


def on_device(*arrays):
    import torch
    return tuple(None if a is None else torch.as_tensor(a, device="cuda") for a in arrays)


def progression(kind):
    if kind == "exact":
        return 37.25 * D + D * np.arange(200)
    j = np.random.default_rng(7).integers(-1, 2, 200).astype(np.float64)      # off the progression by multiples of 2^-34: the first-order term runs
    j[0] = j[-1] = 0.0
    return D * np.arange(1, 201) + j * 2.0 ** -34


def lomb_cases(stage, tag):
    f = _irregular(65)
    for ns in (1, 3):
        t, y, W = record(ns)
        for weights in (True, False):
            td, yd, Wd = stage(t, y, W if weights else None)
            r = L.lombscargle(yd, td, f, W=Wd, path="direct", coef=True, return_sums=True)
            report(f"lombscargle direct ns={ns} W={int(weights)}{tag}", r, L.lombscargle_last_timing())
    td, yd, Wd = stage(*record(3))
    r = L.lombscargle(yd, td, f, W=Wd, path="direct", fit_mean=False, center_data=False, coef=True, return_sums=True)
    report(f"lombscargle direct no mean, not centred{tag}", r, L.lombscargle_last_timing())
    r = L.lombscargle(yd, td, f, W=Wd, path="direct", normalization="psd", coef=True)
    report(f"lombscargle direct psd{tag}", r, L.lombscargle_last_timing())
    os.environ["LPVS_LOMB_BLOCK"] = "64"                                       # 200 frequencies: four blocks per family
    try:
        for kind in ("exact", "rounded"):
            r = L.lombscargle(yd, td, progression(kind), W=Wd, path="nufft", coef=True, return_sums=True)
            tm = L.lombscargle_last_timing()
            assert tm["path"] == "nufft" and tm["blocks"] == (4, 4) and tm["twin"] == (kind == "rounded"), tm
            report(f"lombscargle nufft {kind} grid, blocks of 64{tag}", r, tm)
        td, yd, Wd = stage(*record(130, 300))                                  # two groups of signals: 127 and 3
        r = L.lombscargle(yd, td, progression("exact"), W=Wd, path="nufft", coef=True, return_sums=True)
        report(f"lombscargle nufft ns=130 N=300{tag}", r, L.lombscargle_last_timing())
    finally:
        del os.environ["LPVS_LOMB_BLOCK"]
    for K in (2, 6):
        td, yd, Wd = stage(*record(3))
        r = L.lombscargle(yd, td, _irregular(70, 4), W=Wd, nterms=K, coef=True, return_sums=True)
        report(f"lombscargle nterms={K} ns=3{tag}", r, L.lombscargle_terms_last_timing())


def window_cases(stage, tag):
    t, y, W = record(3)
    f = _irregular(65)
    lo = np.array([-1.0, 10.0, 20.25 + 2.0 ** -12, 39.0, 5.0])                 # the third window lies between two multiples of 2^-10: empty
    hi = np.array([12.0, 30.0, 20.25 + 2.0 ** -11, 41.0, 5.5])
    starts, counts = L.time_windows(stage(t)[0], lo, hi)
    assert (counts == 0).any(), counts
    print(f"{'time_windows' + tag:44s} starts:{sha(starts)} counts:{sha(counts)} | counts={counts.tolist()}", flush=True)
    wins = (starts, counts, lo, hi)
    td, yd, Wd = stage(t, y, W)
    for name, window in (("rect", L.rect), ("hann", L.hanning)):
        r = L.lombscargle_spectrogram(yd, td, f, windows=wins, window=window, W=Wd, coef=True)
        report(f"lombscargle_spectrogram {name}{tag}", r, L.lombscargle_windows_last_timing())
        r = L.lombscargle_welch(yd, td, f, windows=wins, window=window, W=Wd, normalization="psd")
        report(f"lombscargle_welch {name}{tag}", r, L.lombscargle_windows_last_timing())


def wwz_cases(stage, tag):
    t, y, W = record(3)
    f = _irregular(40, 16)
    tau = np.rint(4 * (-0.8 + np.arange(9) * (1.04 * 40 / 8))) / 4
    for name, w, center in (("centred", W, True), ("not centred", W, False), ("zero weights", np.zeros(N), True)):
        td, yd, Wd = stage(t, y, w)
        r = L.wwz(yd, td, f, tau=tau, c=1.0 / (8.0 * np.pi ** 2), W=Wd, center_data=center, coef=True)
        if name == "zero weights":
            assert r[0].empty.all()
        report(f"wwz {name}{tag}", r, L.wwz_last_timing())


def bls_cases(stage, tag):
    """(return_hist=True: the wrapper then passes hist_out, hcount_out and degenerate_out to lpvs_bls_f64)"""
    t, y, W = record(3)
    f = _irregular(70, 4)
    for name, w in (("unit weights", None), ("weights", W)):
        td, yd, Wd = stage(t, y, w)
        r = L.bls(yd, td, f, W=Wd, nbins=100, q=(0.01, 0.1), return_hist=True)
        report(f"bls {name}{tag}", r, L.bls_last_timing())


def bootstrap_cases(stage, tag):
    t, y, W = record(1)
    os.environ["LPVS_LOMB_BOOT_MB"] = "0.01"
    try:
        td, yd, Wd = stage(t, y, W)
        r = L.lombscargle_bootstrap(yd, td, _irregular(70), W=Wd, B=64, seed=5, row0=3, return_argmax=True, return_means=True, return_power=True)
        tm = L.lombscargle_bootstrap_last_timing()
        assert tm["chunks"] > 1, tm
        report(f"lombscargle_bootstrap B=64 row0=3 in chunks{tag}", r, tm)
    finally:
        del os.environ["LPVS_LOMB_BOOT_MB"]


def device_output_cases():
    """lpvs_lombscargle_f64 and lpvs_wwz_f64 with every double output in device memory (the wrappers always pass host arrays)."""
    import torch
    t, y, W = record(3)
    f = _irregular(65)
    Nf, ns = len(f), 3
    ya = np.asfortranarray(y)
    power, coef = torch.zeros(Nf * ns, dtype=torch.float64, device="cuda"), torch.zeros(3 * Nf * ns, dtype=torch.float64, device="cuda")
    ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    _lib.check(_lib.lib().lpvs_lombscargle_f64(_lib.out_ptr(ya), ns, _lib.out_ptr(t), N, _lib.out_ptr(W), _lib.out_ptr(f), Nf, 1, 1, 0, 1, 0, ptr(power), ptr(coef), None))
    torch.cuda.synchronize()
    report("lombscargle direct, device outputs", (power.cpu().numpy(), coef.cpu().numpy()), L.lombscargle_last_timing())
    f = np.ascontiguousarray(_irregular(40, 16))
    tau = np.ascontiguousarray(np.rint(4 * (-0.8 + np.arange(9) * (1.04 * 40 / 8))) / 4)
    c = 1.0 / (8.0 * np.pi ** 2)
    ra = np.ascontiguousarray(L.wwz_radius(f, c, 1e-9))
    Nf, Nt = len(f), len(tau)
    planes = [torch.zeros(ns * Nt * Nf, dtype=torch.float64, device="cuda") for _ in range(3)]
    neff, co = torch.zeros(Nt * Nf, dtype=torch.float64, device="cuda"), torch.zeros(3 * ns * Nt * Nf, dtype=torch.float64, device="cuda")
    counts, empty = np.zeros((Nt, Nf), dtype=np.int64), np.zeros((Nt, Nf), dtype=np.int32)
    _lib.check(_lib.lib().lpvs_wwz_f64(_lib.out_ptr(ya), ns, _lib.out_ptr(t), N, _lib.out_ptr(W), _lib.out_ptr(f), Nf, _lib.out_ptr(tau), Nt, c, _lib.out_ptr(ra), 1, 0,
                                       ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), ptr(neff), ptr(co), _lib.out_ptr(counts), _lib.out_ptr(empty)))
    torch.cuda.synchronize()
    report("wwz centred, device outputs", ([p.cpu().numpy() for p in planes], neff.cpu().numpy(), co.cpu().numpy(), counts, empty), L.wwz_last_timing())


if __name__ == "__main__":
    for stage, tag in ((lambda *a: a, ""), (on_device, ", device inputs")):
        lomb_cases(stage, tag)
        window_cases(stage, tag)
        wwz_cases(stage, tag)
        bls_cases(stage, tag)
        bootstrap_cases(stage, tag)
    device_output_cases()
