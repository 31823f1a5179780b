#!/usr/bin/env python3
"""The ADMM handle through every decision of csrc/admm_plan.h, for comparing two builds of the library (profiles/r11_admm_plan_launches.txt).

    python tools/admm_plan_jobs.py run OUT.npz                       one process: every job below, every returned array into OUT.npz
    python tools/admm_plan_jobs.py compare A.npz B.npz [TRACE_A TRACE_B]
                                                                     arrays bit for bit; with two rocprofv3 --kernel-trace csv files (or the
                                                                     directories that hold them) the library kernels of each stream in sequence

Another build is loaded through LPVS_LIBRARY, in a fresh process per build:
    LPVS_LIBRARY=/path/to/liblpvspectral.so rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/admm_plan_jobs.py run OUT.npz
"""
import collections
import csv
import ctypes
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("LPVS_EXPERIMENTS", "1")

import numpy as np  # noqa: E402

CHUNKS = [10, 6, 1, 110, 1, 127, 1, 200, 144]                # 16, 128, 256 fall on chunk ends, 512 inside a chunk


def run(out_path):
    import torch
    import bench
    import lpvspectral_jl_amd as L
    from lpvspectral_jl_amd._lib import check, lib

    out = {}

    def record(name, p, iters=None):
        x, z, u = p.admm_get(f64=True)
        off = p.admm_get_offset()
        tm = p.timing()
        out[name + "/x"], out[name + "/z"], out[name + "/u"] = x, z, u
        out[name + "/offset"] = np.zeros(0) if off is None else off
        k = ctypes.c_int32(0)
        check(lib().lpvs_admm_matvec_kind(p._h, ctypes.byref(k)))
        out[name + "/counts"] = np.array([k.value, p.time_matvec(2)[1], tm["xcorr_count"], tm["nibble_refreshes"]] +
                                         [v for s in range(p.ns) for v in p.admm_status(s)[::2]] + list(iters or []), dtype=np.float64)

    def solve(name, make, prox, chunks, tol=0.0, mu=0.05, options=(), x0=None):
        with make() as p:
            for k, v in options:
                p.set_option(k, v)
            p.set_prox(prox)
            p.admm_init(x0, μ=mu, tol=tol)
            its = [p.admm_run(c)[0] for c in chunks]
            record(name, p, its)

    dev = torch.device("cuda")
    y, X, V, w = bench.synth_signal(1 << 16, 128, 0, dev)
    lpv = lambda: L.Problem.lpv(y, X, V, w, 8)                # n = 2048
    group = L.SlicedSeparableSum.frequency_groups(5.0, 128, 16)

    # the default handle in the chunking of test_correction_schedule_is_absolute_and_the_offset_is_state; with a stopping test, so that the
    # status is read back after a correction
    solve("default", lpv, group, CHUNKS)
    solve("default_tol", lpv, group, CHUNKS, tol=1e-5)
    for st in ("mixed", "split", "f64"):
        solve("storage_" + st, lpv, group, [70], options=[("storage", st)])
    solve("iteration_two", lpv, group, [70], options=[("iteration", "two")])
    solve("correction_off", lpv, group, [70], options=[("xupdate_correction", "off")])
    solve("prox_l1", lpv, L.NormL1(2.0), [70])
    solve("prox_ball", lpv, L.IndBallL0(40), [40])

    # re-entry at 40 with the offset, then a restart from 0, on one handle; a second init with another mu (new M) and with the same (cached M)
    with lpv() as p:
        p.set_prox(group)
        p.admm_init(None, μ=0.05, tol=0.0)
        p.admm_run(40)
        s40 = p.admm_get() + (p.admm_get_offset(),)
        p.admm_run(30)
        record("state/straight_70", p)
        p.admm_set_state(s40[0], s40[1], s40[2], 40, offset=s40[3])
        p.admm_run(30)
        record("state/reentry_40_with_offset", p)
        p.admm_set_state(s40[0], s40[1], s40[2], 40)
        p.admm_run(30)
        record("state/reentry_40_reformed", p)
        p.admm_set_state(np.zeros_like(s40[0]), np.zeros_like(s40[0]), np.zeros_like(s40[0]), 0)
        p.admm_run(70)
        record("state/restart_0", p)
        p.admm_init(None, μ=0.1, tol=0.0)
        p.admm_run(40)
        record("init/other_mu", p)
        p.admm_init(None, μ=0.1, tol=0.0)
        p.admm_run(40)
        record("init/same_mu", p)

    # two signals; an _f32 handle
    Y2 = torch.stack([y, 0.5 * y], dim=1).contiguous()
    solve("two_signals", lambda: L.Problem.lpv_multi(Y2, X, V, w, 8), group, [40])
    y32, X32, V32, w32 = (a.cpu().numpy().astype(np.float32) for a in (y, X, V, w))
    solve("f32", lambda: L.Problem.lpv(y32, X32, V32, w32, 8), group, [40])

    # N = 2^18: this inverse takes the mixed storage -- the one-launch iteration with the nibble product inside the launches, and on two launches
    yb, Xb, Vb, wb = bench.synth_signal(1 << 18, 128, 0, dev)
    big = lambda: L.Problem.lpv(yb, Xb, Vb, wb, 8)
    solve("mixed_one_launch", big, group, [1, 31, 1, 5, 26, 6, 130])
    solve("mixed_one_launch_tol", big, group, [200], tol=1e-3)
    solve("mixed_two_launches", big, group, [70], options=[("iteration", "two")])
    solve("mixed_36_bit_reads", big, group, [70], options=[("storage", "mixed")])

    # the Fourier handle whose tiles are all fixed point (test_stale_nibble_product_on_a_fourier_handle_whose_tiles_are_all_fixed_point)
    rng = np.random.default_rng(23)
    N, Nf = 1 << 15, 1024
    t = np.arange(N, dtype=np.float64)
    f = (np.arange(Nf) + 0.5) / (2.0 * Nf + 1.0)
    yf = np.sin(2 * np.pi * f[100] * t) + 0.5 * np.cos(2 * np.pi * f[700] * t) + 0.2 * rng.standard_normal(N)
    solve("fourier_all_fixed", lambda: L.Problem.fourier(yf, t, f), L.NormL1(30.0), [1, 15, 16, 1, 31, 26])

    # an explicit Gram of n = 2048 whose inverse is not diagonally dominant (half the spectrum far above 1 / mu): the mixed packing is
    # demoted to split; the second init finds the demoted copy and does not pack again
    U = rng.standard_normal((2048, 1024))
    G = U @ U.T
    b = rng.standard_normal(2048)
    with L.Problem.gram(G, b) as p:
        p.set_prox(L.NormL1(0.01))
        for name in ("demoted/first_init", "demoted/second_init"):
            p.admm_init(None, μ=0.05, tol=0.0)
            p.admm_run(40)
            record(name, p)

    # n = 1024: graph replays plus a remainder, the same launch by launch, and a group length the small kernel refuses (two launches)
    Ns, Nfs = 1 << 13, 64
    ts = np.sort(rng.random(Ns)) * Ns
    fs = (np.arange(Nfs) + 0.5) / (2.0 * Nfs + 1.0)
    ys = np.sin(2 * np.pi * fs[10] * ts) + 0.3 * rng.standard_normal(Ns)
    ws = 2 * np.pi * fs
    Vs = np.linspace(0, 1, Ns)
    small = lambda: L.Problem.lpv(ys, ts, Vs, ws, 8)          # n = 2 * 64 * 8 = 1024
    solve("small_graph", small, L.NormL1(1.0), [600])
    solve("small_two_calls", small, L.NormL1(1.0), [100, 500])
    os.environ["LPVS_NO_GRAPH"] = "1"
    solve("small_no_graph", small, L.NormL1(1.0), [600])
    del os.environ["LPVS_NO_GRAPH"]
    solve("small_group_16", small, L.SlicedSeparableSum.frequency_groups(1.0, Nfs, 16), [120])
    solve("small_group_512", small, L.SlicedSeparableSum.frequency_groups(1.0, 2, 512), [120])      # > 256: the small kernel refuses it
    solve("small_iteration_two", small, L.NormL1(1.0), [120], options=[("iteration", "two")])

    np.savez(out_path, **out)
    print(f"{len(out)} arrays of {len({k.rsplit('/', 1)[0] for k in out})} runs -> {out_path}")


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def library_launches(path):
    """{stream or queue: [(kernel, grid, workgroup, static LDS), ...] in dispatch order}, and the count of the runtime's own kernels."""
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r.get("Start_Timestamp") or 0))
    per, runtime = collections.defaultdict(list), 0
    for r in rows:
        name = r.get("Kernel_Name", "")
        if "lpvs::" not in name:
            runtime += name.startswith("__amd_rocclr")
            continue
        sig = (name, tuple(r.get("Grid_Size_" + a, "") for a in "XYZ"), tuple(r.get("Workgroup_Size_" + a, "") for a in "XYZ"), r.get("LDS_Block_Size", ""))
        per[r.get("Stream_Id") or r.get("Queue_Id") or "0"].append(sig)
    return per, runtime


def compare(a_path, b_path, traces):
    a, b = np.load(a_path), np.load(b_path)
    bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or a[k].shape != b[k].shape
           or a[k].tobytes() != b[k].tobytes()]
    print(f"outputs: {len(a.files)} arrays against {len(b.files)}: " + ("all equal bit for bit" if not bad else "DIFFERENT: " + ", ".join(bad)))
    ok = not bad
    if traces:
        (la, ra), (lb, rb) = library_launches(traces[0]), library_launches(traces[1])
        seq_a, seq_b = sorted(la.values(), key=len), sorted(lb.values(), key=len)   # (stream ids are handed out per process: match by content)
        same_seq = sorted(map(tuple, seq_a)) == sorted(map(tuple, seq_b))
        count = lambda l: collections.Counter(s for v in l.values() for s in v)
        na, nb = sum(map(len, seq_a)), sum(map(len, seq_b))
        print(f"library kernels {na} against {nb} on {len(seq_a)} / {len(seq_b)} streams ({[len(s) for s in seq_a]} per stream), "
              f"{len(count(la))} distinct (kernel, grid, workgroup, static LDS);")
        print(f"  sequence of launches on each stream {'EQUAL' if same_seq else 'DIFFERENT'}, multiset {'EQUAL' if count(la) == count(lb) else 'DIFFERENT'}; "
              f"the runtime's own copy / fill kernels (__amd_rocclr_*): {ra} against {rb}")
        if not same_seq:
            for sa, sb in zip(seq_a, seq_b):
                first = next((i for i, (p, q) in enumerate(zip(sa, sb)) if p != q), min(len(sa), len(sb)))
                print(f"  first difference at launch {first}: {sa[first:first + 1]} against {sb[first:first + 1]}")
        names = collections.Counter(s[0].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for v in lb.values() for s in v)
        print("library kernels of the second run, launches per kernel:")
        for name, c in sorted(names.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"  {c:6d}  {name}")
        ok = ok and same_seq
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) in (4, 6) and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:6]))
    else:
        sys.exit(__doc__)
