"""No result depends on what a reused device block held ("Every byte a kernel reads was written in the same call").

Every workspace of the library comes from one caching allocator (csrc/api.hip: DevBuf::alloc) that hands freed blocks out again, never
cleared and up to 25 % + 1 MiB larger than asked for.  The experiment knob LPVS_POOL_FILL=<two hex digits> fills every block over its whole
true size before it is handed out, and asks for fresh blocks with a slack, so that their true size exceeds the request as a reused block's
does.  Every case below is ONE call of the library in fresh handles; it runs with the knob unset and with the bytes

    00   what a fresh driver block usually looks like,
    ff   a NaN as a double and as a float, -1 as an int32, the maximum of an unsigned 64-bit accumulator: a missing zero fill of a sum, a
         ticket or an atomicMax cell cannot hide behind it,
    55   a finite 1.19e103 as a double, 1.5e13 as a float, a large positive integer: a read that a NaN-tolerant reduction (a maximum, a
         `> 0` guard) would swallow,

and the four results must be EQUAL BYTE FOR BYTE: every returned array through .view(uint8) (NaN positions and signed zeros count), every
scalar and iteration count, and of the timing dicts every field that names a path, form, storage or plan -- only the times (*_ms, *_us) are
left out.  All accumulation in the library is in a fixed order or in integer atomics, so no tolerance is needed and none is used.  The inputs
are those of the smallest case with which the feature's own GPU test reaches the path, and the path is asserted where the library reports it.

test_features_interleaved_forward_and_backward runs every case once in the listed order and once in reverse in one process with NO knob:
blocks reused across features, the production situation.  GPU only."""
import ctypes as C
import functools
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gram_ref as GR  # noqa: E402
import _dense_ref as DR  # noqa: E402

pytestmark = pytest.mark.gpu

KNOB = "LPVS_POOL_FILL"
FILLS = (None, "00", "ff", "55")
OPTION_ENV = ("LPVS_M_STORAGE", "LPVS_ITERATION", "LPVS_GRAM_FORM", "LPVS_NUDFT", "LPVS_NUFFT_SPREAD", "LPVS_NT_LOADS", "LPVS_WINDOW_CHUNK_MB", "LPVS_WINDOWS_IN_FLIGHT",
              "LPVS_LOMB_BLOCK", "LPVS_LOMB_BOOT_MB", "LPVS_LOMB_BOOT_TS", "LPVS_NO_GRAPH", "LPVS_WINDOW_MATVEC_TIMING")


# ---- the helper --------------------------------------------------------------------------------------------------------------------------
def _is_time(key):
    return key.endswith("_ms") or key.endswith("_us") or "us_per" in key


def _flat(obj, prefix="", out=None):
    """Every array, scalar and plan field of a result as {path: ndarray}: tuples, lists and dicts by index / key, result objects by their
    attributes, device tensors copied to the host; the time fields of the timing dicts are dropped (nothing else is)."""
    out = {} if out is None else out
    if obj is None:
        out[prefix] = np.zeros(0)
    elif hasattr(obj, "detach"):
        out[prefix] = np.ascontiguousarray(obj.detach().cpu().numpy())
    elif isinstance(obj, np.ndarray):
        out[prefix] = np.ascontiguousarray(obj)
    elif isinstance(obj, dict):
        for k in sorted(obj):
            if not _is_time(str(k)):
                _flat(obj[k], f"{prefix}.{k}", out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _flat(v, f"{prefix}[{i}]", out)
    elif isinstance(obj, (bool, int, float, complex, str, np.generic)):
        out[prefix] = np.asarray(obj) if not isinstance(obj, str) else np.frombuffer(obj.encode(), dtype=np.uint8)
    elif isinstance(obj, range):
        out[prefix] = np.asarray(list(obj))
    elif hasattr(obj, "__dict__"):
        for k, v in sorted(vars(obj).items()):
            if not callable(v):
                _flat(v, f"{prefix}.{k}", out)
    else:
        raise TypeError(f"{prefix}: a {type(obj).__name__} cannot be compared")
    return out


def _differences(a, b):
    """The paths at which two flattened results differ in a byte, shape or type (empty: equal)."""
    bad = []
    if sorted(a) != sorted(b):
        return [f"the results have other fields: {sorted(set(a) ^ set(b))}"]
    for k in a:
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            bad.append(f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}")
        elif x.dtype == object:
            if not all(u == v for u, v in zip(x.ravel(), y.ravel())):
                bad.append(f"{k}: objects differ")
        elif x.tobytes() != y.tobytes():
            xb, yb = (a.reshape(-1).view(np.uint8).reshape(a.size, -1) for a in (x, y))
            ne = np.flatnonzero((xb != yb).any(axis=1))
            bad.append(f"{k}: {len(ne)} of {x.size} elements differ, first at flat index {int(ne[0])}: {x.reshape(-1)[ne[0]]!r} against {y.reshape(-1)[ne[0]]!r}")
    return bad


def _run(case, L, monkeypatch, fill):
    for v in OPTION_ENV:
        monkeypatch.delenv(v, raising=False)
    if fill is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, fill)
    assert os.environ.get("LPVS_EXPERIMENTS") == "1", "the knob is inert without the master switch (tests/conftest.py sets it)"
    r = _flat(case(L, monkeypatch))
    monkeypatch.delenv(KNOB, raising=False)
    assert r, "the case returned nothing to compare"
    return r


def same_bytes_whatever_the_block_held(case, L, monkeypatch, fills=None):
    """THE helper: the case's call in fresh handles once per fill; every result equals the first one byte for byte."""
    fills = FILLS if fills is None else fills
    first = _run(case, L, monkeypatch, fills[0])
    for fill in fills[1:]:
        bad = _differences(first, _run(case, L, monkeypatch, fill))
        assert not bad, f"{KNOB}={fill} against {fills[0] or 'unset'}: " + "; ".join(bad[:8])


def _unfilled(fn):
    """Inputs that come from the library itself (an estimate the case starts from) are computed once, with the knob off -- taking it out of
    os.environ is enough, the library reads it at every allocation.  The cached estimate is shared by all fills, so the ComplexNormal cases do
    NOT run ls_spectral_lpv under a fill: the ls_spectral_lpv-* cases do."""
    @functools.lru_cache(maxsize=None)
    def cached(*args):
        old = os.environ.pop(KNOB, None)
        try:
            return fn(*args)
        finally:
            if old is not None:
                os.environ[KNOB] = old
    return cached


CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return reg


# ---- structured Gram (tests/test_gpu_nufft_gather.py) ---------------------------------------------------------------------------------------
D_STEP = 0.731


def _ap_data(N, Nf, ns=1, seed=None):
    rng = np.random.default_rng(N if seed is None else seed)
    X = np.sort(rng.random(N) * 400.0 - 100.0)
    V = rng.random(N) * 2 - 0.5
    w = D_STEP * (1.0 + np.arange(Nf))
    Y = rng.standard_normal(N) if ns == 1 else rng.standard_normal((N, ns))
    return Y, X, V, w


def _handle_outputs(p):
    Gt, bt = p.device_gram()
    tm = p.timing()
    return dict(gram=p.get_gram(), rhs=p.get_rhs(), device_gram=Gt.cpu().numpy().copy(), device_rhs=bt.cpu().numpy().copy(), timing=tm, n=p.n)


def _structured(N, Nf, Nv, ns, env, form, n=None):
    def run(L, mp):
        for k, v in env.items():
            mp.setenv(k, v)
        Y, X, V, w = _ap_data(N, Nf, ns, seed=Nf if n else None)
        with (L.Problem.lpv_multi(Y, X, V, w, Nv) if ns > 1 else L.Problem.lpv(Y, X, V, w, Nv)) as p:
            r = _handle_outputs(p)
        assert r["timing"]["gram_form"] == form and (n is None or r["n"] == n), (r["timing"], r["n"])
        return r
    return run


CASES["gram-ap-nufft-4096x24x3"] = _structured(4096, 24, 3, 1, {}, "ap-nufft")
CASES["gram-ap-direct-4096x24x3"] = _structured(4096, 24, 3, 1, {"LPVS_NUDFT": "direct"}, "ap")
CASES["gram-ap-nufft-scatter-4096x24x3"] = _structured(4096, 24, 3, 1, {"LPVS_NUFFT_SPREAD": "scatter"}, "ap-nufft")
CASES["gram-ap-nufft-n222-in-256"] = _structured(4096, 37, 3, 1, {}, "ap-nufft", n=222)
CASES["gram-ap-nufft-n260-in-384"] = _structured(4096, 65, 2, 1, {}, "ap-nufft", n=260)
CASES["gram-ap-nufft-multi3-6000x20x3"] = _structured(6000, 20, 3, 3, {}, "ap-nufft")


# ---- dense Gram (tests/_gram_ref.py, tests/test_gpu_gram_dense.py) ---------------------------------------------------------------------------
def _dense_lpv(cid):
    c = {x[0]: x for x in GR.LPV_CASES}[cid]

    def run(L, mp):
        y, X, V, w = GR.lpv_inputs(c)
        with L.default_options(gram_form=c[4]):
            with L.Problem.lpv(y, X, V, w, c[2], normalize=c[7]) as p:
                r = _handle_outputs(p)
        assert r["timing"]["gram_form"] == c[5] and r["timing"]["gram_stage"] == c[6], r["timing"]
        if c[3] == 333:
            assert r["timing"]["gram_ksplit"] == 1                                    # one chunk of 384 rows: 51 pad rows
        return r
    return run


for _cid in ("krs-70x2-N333", "krs-8x20", "kr-22x7-N333", "kr-20x8", "kr-1x640"):
    CASES[f"gram-dense-{_cid}"] = _dense_lpv(_cid)


@case("gram-dense-panel-339-W-N333")
def _panel(L, mp):
    c = {x[0]: x for x in GR.FOURIER_CASES}["panel-339-W-N333"]
    y, t, f, W = GR.fourier_inputs(c)
    with L.Problem.fourier(y, t, f, W) as p:
        r = _handle_outputs(p)
    assert r["timing"]["gram_form"] == "panel" and r["n"] == 339, r["timing"]
    return r


# ---- factorisation and solves ------------------------------------------------------------------------------------------------------------------
def _solves(Nf, Nv, n):
    def run(L, mp):
        Y, X, V, w = _ap_data(4096, Nf, 1, seed=Nf)
        out = {}
        for name, call in (("inverse", lambda p: p.get_inverse(20.0)), ("inverse_refined", lambda p: p.get_inverse_refined(20.0)), ("ridge", lambda p: p.solve_ridge(1e-3))):
            with L.Problem.lpv(Y, X, V, w, Nv) as p:                                  # a fresh handle per solve
                assert p.n == n
                out[name] = call(p)
                out[name + "_timing"] = p.timing()
        return out
    return run


CASES["solves-n222"] = _solves(37, 3, 222)
CASES["solves-n260"] = _solves(65, 2, 260)


def _ls_spectral(cid):
    def run(L, mp):
        y, t, f, W, _ = DR.primal_inputs(DR.PRIMAL[cid])
        return L.ls_spectral(y, t, f, W, λ=DR.PRIMAL[cid][5])
    return run


CASES["ls_spectral-n127-N333"] = _ls_spectral("n127-N333")
CASES["ls_spectral-n127-N333-W"] = _ls_spectral("n127-N333-W")
CASES["ls_spectral-n129-N333-W-ap"] = _ls_spectral("n129-N333-W-ap")


@case("ls_spectral-dual-N=3")
def _ls_spectral_dual(L, mp):
    y, t, f = DR.dual_inputs(next(c for c in DR.DUAL_CASES if c[0] == "N=3"))
    return L.ls_spectral(y, t, f, λ=DR.DUAL_LAM)


@case("tls_spectral-n127-N333")
def _tls(L, mp):
    y, t, f, _, _ = DR.primal_inputs(DR.PRIMAL["n127-N333"])
    return L.tls_spectral(y, t, f)


def _ls_spectral_lpv(cid):
    def run(L, mp):
        _, Nf, Nv, N, coulomb, normalize, prog, lam = DR.LPV[cid]
        Y, X, V, w = DR.lpv_inputs(DR.LPV[cid])
        out = {}
        for cov in (False, True):
            se = L.ls_spectral_lpv(Y, X, V, w, Nv, λ=lam, coulomb=coulomb, normalize=normalize, covariance=cov)
            out[f"x{int(cov)}"], out[f"sigma{int(cov)}"] = np.asarray(se.x), (None if se.Σ is None else np.asarray(se.Σ))
        return out
    return run


CASES["ls_spectral_lpv-krs-9x8"] = _ls_spectral_lpv("krs-9x8")                       # n = 144: one pad strip of 112
CASES["ls_spectral_lpv-ap-10x3"] = _ls_spectral_lpv("ap-10x3")


# ---- ADMM -----------------------------------------------------------------------------------------------------------------------------------
def _admm_outputs(p, iters=60):
    p.admm_init(None, μ=0.05, tol=0.0)
    info = p.matvec_info()
    ran = p.admm_run(iters)
    return dict(ran=ran, state=p.admm_get(), status=[p.admm_status(q) for q in range(p.ns)], offset=p.admm_get_offset(), kernel=info["kernel"],
                storage=info.get("storage", ""), one_launch=info.get("one_launch_iteration", False), timing=p.timing())


def _admm_n222(prox, iteration=None, kernel="admm_small_iter_kernel"):
    def run(L, mp):
        Y, X, V, w = _ap_data(4096, 37, 1, seed=37)
        with L.Problem.lpv(Y, X, V, w, 3) as p:
            assert p.n == 222
            if iteration:
                p.set_option("iteration", iteration)
            p.set_prox(prox(L))
            r = _admm_outputs(p)
        assert r["kernel"] == kernel and r["status"][0][0] == 60, (r["kernel"], r["status"])
        return r
    return run


CASES["admm-n222-l1"] = _admm_n222(lambda L: L.NormL1(0.5))
CASES["admm-n222-l0"] = _admm_n222(lambda L: L.NormL0(0.02))
CASES["admm-n222-ball-l0"] = _admm_n222(lambda L: L.IndBallL0(20), None, "symv_kernel")       # (the selection has no one-launch form)
CASES["admm-n222-group"] = _admm_n222(lambda L: L.SlicedSeparableSum.frequency_groups(5.0, 37, 6))
CASES["admm-n222-group-two-launches"] = _admm_n222(lambda L: L.SlicedSeparableSum.frequency_groups(5.0, 37, 6), "two", "symv_kernel")


def _signal_2048(N, Nf, rng):                                                           # tests/test_gpu_options.py, tests/test_gpu_one_launch.py
    X = np.sort(rng.random(N) * (10.0 * N / 500)); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
    y = 2 * V ** 2 * np.cos(w[Nf // 10] * X) + 2 / (5 * V + 1) * np.cos(w[Nf // 3] * X - 0.3) + 0.1 * rng.standard_normal(N)
    return y, X, V, w


@functools.lru_cache(maxsize=None)
def _sig_2048():
    return _signal_2048(1 << 18, 128, np.random.default_rng(3))                         # n = 2048: the smallest size with a packed inverse


def _admm_2048(storage, iteration, kernel, reads32, prox="group"):
    def run(L, mp):
        y, X, V, w = _sig_2048()
        proxes = {"group": L.SlicedSeparableSum.frequency_groups(2.0, 128, 16), "l1": L.NormL1(0.5), "l0": L.NormL0(0.02)}
        with L.Problem.lpv(y, X, V, w, 8) as p:
            p.set_prox(proxes[prox])
            p.set_option("storage", storage); p.set_option("iteration", iteration)
            r = _admm_outputs(p)
        assert r["kernel"] == kernel, (storage, iteration, r["kernel"])
        assert reads32 is None or ("32-bit fixed point reads" in r["storage"]) == reads32, (storage, r["storage"])
        return r
    return run


CASES["admm-n2048-default-one-launch"] = _admm_2048(None, None, "admm_iter_mixed_kernel", True)
CASES["admm-n2048-two-launches"] = _admm_2048(None, "two", "symv_tile_mixed_kernel", None)
CASES["admm-n2048-f64"] = _admm_2048("f64", None, "symv_tile_kernel<double>", False)
CASES["admm-n2048-split"] = _admm_2048("split", None, "symv_tile_split_kernel", False)
CASES["admm-n2048-mixed"] = _admm_2048("mixed", "one", "admm_iter_mixed_kernel", False)
CASES["admm-n2048-mixed32"] = _admm_2048("mixed32", None, "admm_iter_mixed_kernel", True)
CASES["admm-n2048-one-launch-l1"] = _admm_2048(None, None, "admm_iter_mixed_kernel", True, "l1")
CASES["admm-n2048-one-launch-l0"] = _admm_2048(None, None, "admm_iter_mixed_kernel", True, "l0")


def _admm_small_fourier(zero, iteration, kernel):                                       # tests/test_gpu_small_one_launch.py
    def run(L, mp):
        rng = np.random.default_rng(71)
        N, Nf = 1500, 512
        t = np.sort(rng.random(N)) * N
        f = (np.arange(Nf) if zero else np.arange(1, Nf + 1)) / (2.0 * Nf)
        y = 2 * np.sin(2 * np.pi * f[16] * t + 0.3) + np.sin(2 * np.pi * f[99] * t) + 0.25 * np.sin(2 * np.pi * f[300] * t + 1.0) + 0.1 * rng.standard_normal(N)
        with L.Problem.fourier(y, t, f) as p:
            assert p.n == (1023 if zero else 1024)
            if iteration:
                p.set_option("iteration", iteration)
            p.set_prox(L.NormL1(0.05))
            r = _admm_outputs(p)
        assert r["kernel"] == kernel, r["kernel"]
        return r
    return run


CASES["admm-small-n1024"] = _admm_small_fourier(False, None, "admm_small_iter_kernel")
CASES["admm-small-n1023-zero-frequency"] = _admm_small_fourier(True, None, "admm_small_iter_kernel")
CASES["admm-small-n1024-two-launches"] = _admm_small_fourier(False, "two", "symv_kernel")


@case("admm-multi3-6000x20x3")
def _admm_multi(L, mp):
    Y, X, V, w = _ap_data(6000, 20, 3)
    with L.Problem.lpv_multi(Y, X, V, w, 3) as p:
        p.set_prox(L.SlicedSeparableSum.frequency_groups(5.0, 20, 6))
        r = _admm_outputs(p)
    assert r["kernel"] == "admm_small_iter_kernel" and [s[0] for s in r["status"]] == [60, 60, 60], (r["kernel"], r["status"])
    return r


@case("admm-f32-5000x128x8")
def _admm_f32(L, mp):                                                                    # tests/test_gpu_f32.py: the single-precision matrix is streamed
    rng = np.random.default_rng(21)
    N, Nf, Nv = 5000, 128, 8
    X = np.sort(rng.random(N) * 10 * N / 500).astype(np.float32)
    V = np.linspace(0, 1, N).astype(np.float32)
    w = (2 * np.pi * (np.arange(Nf) + 1.0) * 25 / Nf / 4).astype(np.float32)
    y = (2 * V ** 2 * np.cos(w[12] * X) + 2 / (5 * V + 1) * np.cos(w[60] * X) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    with L.Problem.lpv(y, X, V, w, Nv) as p:
        p.set_prox(L.SlicedSeparableSum.frequency_groups(3.0, Nf, 2 * Nv))
        r = _admm_outputs(p)
        r["state64"] = p.admm_get(f64=True)
    assert r["kernel"] == "admm_iter_mixed_kernel" and r["one_launch"], (r["kernel"], r["storage"])      # n = 2048: the single-precision copy, one launch
    assert r["state"][0].dtype == np.float32 and r["status"][0][0] == 60
    return r


def _admm_f32_2048(iteration, kernel):                                                   # tests/test_gpu_one_launch.py: _f32 handles at n = 2048
    def run(L, mp):
        y, X, V, w = (a.astype(np.float32) for a in _signal_2048(1 << 18, 128, np.random.default_rng(21)))
        with L.Problem.lpv(y, X, V, w, 8) as p:
            assert p.f32
            p.set_option("iteration", iteration)
            p.set_prox(L.SlicedSeparableSum.frequency_groups(2.0, 128, 16))
            r = _admm_outputs(p)
            r["state64"] = p.admm_get(f64=True)
        assert r["kernel"] == kernel and r["one_launch"] == (iteration is None) and r["status"][0][0] == 60, (r["kernel"], r["status"])
        return r
    return run


CASES["admm-f32-n2048-one-launch"] = _admm_f32_2048(None, "admm_iter_mixed_kernel")
CASES["admm-f32-n2048-two-launches"] = _admm_f32_2048("two", "symv_tile_f32_kernel")


@case("admm-path-4-points-n222")
def _admm_path(L, mp):
    Y, X, V, w = _ap_data(4096, 37, 1, seed=37)
    ses = L.ls_sparse_spectral_lpv_path(Y, X, V, w, 3, nλ=4, iters=60, tol=0.0, printerval=1000, out=io.StringIO())
    assert len(ses) == 4
    return [(se.x, se.λ) for se in ses]


# ---- window engine ---------------------------------------------------------------------------------------------------------------------------
def _engine(L, sparse):
    from lpvspectral_jl_amd import _lib
    if sparse:
        return dict(estimator=_lib.EST_SPARSE, lam=0.0, prox=(_lib.PROX_L1, 0.3, 0), μ=0.01, tol=0.0, iters=200, sign=_lib.LINEAR_LEAST_SQUARES)
    return dict(estimator=_lib.EST_DENSE, lam=1e-4, prox=(_lib.PROX_L1, 0.0, 0), μ=0.05, tol=0.0, iters=0, sign=_lib.LINEAR_LEAST_SQUARES)


def _nufft_windows():                                                                    # tests/test_gpu_nufft.py: n = 4096, 6 windows, Nf = 96, two signals, Hann
    rng = np.random.default_rng(2)
    n, nwin, Nf = 4096, 6, 96
    Ltot = n * nwin
    t = np.arange(Ltot) * 0.5 + 0.01 * rng.random(Ltot)
    f = np.arange(Nf) / (2.0 * Nf)
    Ys = [np.ascontiguousarray(np.sin(2 * np.pi * f[7 + 3 * q] * t) + 0.3 * rng.standard_normal(Ltot)) for q in range(2)]
    return n, t, f, Ys, np.hanning(n) + 0.1


def _windows_nufft(sparse, shard=None, csd=False):
    def run(L, mp):
        n, t, f, Ys, W = _nufft_windows()
        eng = _engine(L, sparse)
        kw = {} if shard is None else dict(win_lo=shard[0], win_hi=shard[1])
        r = L.windowcsd_batched(Ys[0], Ys[1], t, f, n, 0, W, eng, **kw) if csd else L.windows_estimate(Ys, t, f, n, 0, W, eng, **kw)
        tm = L.windowpsd_last_timing()
        assert tm["gram_form"] == "ap-nufft" and tm["windows"] == (6 if shard is None else shard[1] - shard[0]), tm
        return r, tm
    return run


CASES["windows-nufft-sparse"] = _windows_nufft(True)
CASES["windows-nufft-dense"] = _windows_nufft(False)
CASES["windows-nufft-sparse-shard-2-5"] = _windows_nufft(True, (2, 5))
CASES["windowcsd-nufft-sparse"] = _windows_nufft(True, csd=True)
CASES["windowcsd-nufft-dense-shard-2-5"] = _windows_nufft(False, (2, 5), csd=True)


def _windows_ragged(sparse):                                                             # tests/test_gpu_edges.py: a ragged tail, overlapping Hann windows
    def run(L, mp):
        rng = np.random.default_rng(5)
        Ltot, nw, noverlap = 5000, 9, 100
        t = np.arange(Ltot) * 0.5
        y = np.sin(2 * np.pi * 0.11 * t) + 0.5 * np.sin(2 * np.pi * 0.31 * t) + 0.2 * rng.standard_normal(Ltot)
        u = np.cos(2 * np.pi * 0.11 * t + 0.4) + 0.2 * rng.standard_normal(Ltot)
        f = np.arange(0, 40) / 80.0
        n = Ltot // nw                                                                   # as ls_windowpsd: ten windows of 555 and a tail that fits none
        eng = dict(_engine(L, sparse), iters=300 if sparse else 0, μ=0.05)
        r = L.windows_estimate([y, u], t, f, n, noverlap, L.hanning(n), eng)
        tm = L.windowpsd_last_timing()
        assert tm["windows"] == (Ltot - n) // (n - noverlap) + 1 and (Ltot - n) % (n - noverlap) != 0, tm
        return r, tm, L.windowcsd_batched(y, u, t, f, n, noverlap, L.hanning(n), eng)
    return run


CASES["windows-ragged-overlap-sparse"] = _windows_ragged(True)
CASES["windows-ragged-overlap-dense"] = _windows_ragged(False)


def _windows_np512(iteration):
    """tests/test_gpu_one_launch.py::test_padded_and_stiff_problems_keep_the_quantum_tight: nreg = 511 in np = 512, six windows -- the batch's
    one-launch iteration with its accumulator block (fibuf), against the two-launch scheme."""
    def run(L, mp):
        from lpvspectral_jl_amd import _lib
        rng = np.random.default_rng(5)
        n, nwin, Nfw = 1 << 14, 6, 256
        t = np.arange(n * nwin, dtype=np.float64)
        f = np.arange(Nfw) / 512.0
        yw = np.sin(2 * np.pi * f[33] * t) + 0.5 * np.sin(2 * np.pi * f[100] * t) + 0.3 * rng.standard_normal(n * nwin)
        eng = dict(estimator=_lib.EST_SPARSE, lam=0.0, prox=(_lib.PROX_L1, 0.2, 0), μ=1e-4, tol=0.0, iters=300, sign=_lib.LINEAR_QUADRATIC_AS_WRITTEN)
        with L.default_options(iteration=iteration):
            r = L.windows_estimate([yw], t, f, n, 0, None, eng)
        tm = L.windowpsd_last_timing()
        assert tm["one_launch_iteration"] == (iteration is None) and tm["windows"] == 6, tm
        return r, tm
    return run


CASES["windows-np512-one-launch"] = _windows_np512(None)
CASES["windows-np512-two-launches"] = _windows_np512("two")


@case("windows-f32-chunked-plan")
def _windows_f32_chunked(L, mp):
    """tests/test_gpu_f32.py::test_f32_window_calls_take_the_chunked_plan: 1 MB chunks, three parts in flight -- the packing of a batch's inverses
    (mixed against split) was decided from the TRUE size of the block."""
    rng = np.random.default_rng(61)
    n, nwin, Nf = 1 << 10, 40, 64
    t = np.arange(n * nwin, dtype=np.float32)
    f = (np.arange(Nf) / 128.0).astype(np.float32)
    y = (np.sin(2 * np.pi * f[9].astype(np.float64) * t.astype(np.float64)) + 0.3 * rng.standard_normal(n * nwin)).astype(np.float32)
    eng = dict(estimator=1, lam=0.0, prox=(1, 0.3, 0), μ=1e-3, tol=0.0, iters=100, sign=-1)
    with L.default_options(window_chunk_mb=1, windows_in_flight=3):
        x, its = L.windows_estimate([y], t, f, n, 0, None, eng)
    tm = L.windowpsd_last_timing()
    assert x.dtype == np.complex64 and tm["gram_form"] in ("ap", "ap-nufft") and tm["windows"] == 40, tm
    assert tm["passes"] > 1, tm                                                          # the plan was cut: several chunks / parts, a pass each
    assert tm["one_launch_iteration"], tm                                                # the mixed packing ran: only it leads to the one-launch iteration
    return x, its, tm


# ---- predict / residual / fva (tests/test_gpu_predict.py) ----------------------------------------------------------------------------------
def _coefs(rng, n, nc=1):
    return (rng.standard_normal((n, nc)) + 1j * rng.standard_normal((n, nc))) * 10.0 ** rng.integers(-2, 2, (n, 1))


def _plant(x, period):
    x[:4] = [0.0, period * (1e-9 / (2 * np.pi)) + 3 * period, period * (1 - 1e-9 / (2 * np.pi)) + period, 0.5 * period + 2 * period]
    return x


def _eval_outputs(L, args, y_args, path, want):
    out = {"predict": L.predict(*args, path=path)}
    tm = L.eval_last_timing()
    assert tm["path"] == want, tm
    out["predict_timing"] = tm
    out["residual"] = L.residual(*y_args, path=path, return_sums=True)
    out["residual_timing"] = L.eval_last_timing()
    out["fva"] = L.fva(*y_args, path=path)
    return out


def _predict_lpv(path):
    def run(L, mp):
        if path == "direct":                                                             # Nf = 24, Nv = 3, no progression, M = 4099: 17 slabs, the last of 3
            rng = np.random.default_rng(31 + 2)
            M = 4099
            X, V = rng.uniform(-3.0, 5.0, M), rng.uniform(-1.0, 1.0, M)
            w = np.sort(rng.uniform(0.4, 6.0, 24))
        else:                                                                            # "ap-24x3": a progression, M = 4099, the 256 grid
            rng = np.random.default_rng(900 + 24 + 3 + 1)
            M = 4096 + 3
            X = _plant(rng.permutation(np.sort(rng.random(M)) * 50.0), 7.0)
            V = rng.uniform(-1.0, 1.0, M)
            w = (2 * np.pi / 7.0) * np.arange(1, 25)
        P = _coefs(rng, 24 * 3, 2)
        se = L.SpectralExt(rng.standard_normal(M), X, V, w, 3, 1.0, False, True, P, None)
        r = _eval_outputs(L, (se,), (se,), "auto", path)
        assert r["predict_timing"]["slabs"] == 17 if path == "direct" else r["predict_timing"]["nf"] == 256, r["predict_timing"]
        return r
    return run


def _predict_fourier(path):
    def run(L, mp):
        if path == "direct":
            rng = np.random.default_rng(41)
            M = 1000
            t = np.cumsum(0.5 + rng.random(M))
            f = np.sort(rng.uniform(0.01, 0.45, 40))
        else:                                                                            # "ap-fourier": k / 97, M = 4099
            rng = np.random.default_rng(17 + len("ap-fourier"))
            M = 4096 + 3
            f = np.arange(1, 41) / 97.0
            t = np.sort(_plant(np.sort(rng.random(M) * 300.0), 97.0))
        p = _coefs(rng, 40)[:, 0]
        y = rng.standard_normal(M)
        return _eval_outputs(L, (p, f, t), (p, f, t, y), "auto", path)
    return run


CASES["predict-lpv-direct"] = _predict_lpv("direct")
CASES["predict-lpv-nufft"] = _predict_lpv("nufft")
CASES["predict-fourier-direct"] = _predict_fourier("direct")
CASES["predict-fourier-nufft"] = _predict_fourier("nufft")


# ---- ComplexNormal (tests/test_gpu_cnormal.py) -----------------------------------------------------------------------------------------------
@_unfilled
def _lpv_estimate(Nv):
    """The LPV test problem of tests/_cnormal_ref.py and its ridge estimate with covariance (an INPUT of the cases: computed once, knob off)."""
    import lpvspectral_jl_amd as L
    import _cnormal_ref as CR
    Y, V, X, _, _ = CR.generate_signal(CR.F_TRUE, 2 * np.pi * np.array([2.0, 10.0, 20.0]), 500, True, seed=0)
    return L.ls_spectral_lpv(Y, X, V, 2 * np.pi * np.arange(2, 25, 2.0), Nv, λ=0.02, normalize=True, coulomb=False)


@case("cnormal-cholesky-n2-130")
def _chol(L, mp):
    rng = np.random.default_rng(130)
    A = rng.standard_normal((130, 130))
    return L.cholesky_upper(A.T @ A / 130 + np.eye(130))                               # (cn_last_timing's n2 / draws are those of the last rand: not this call's)


@case("cnormal-rand-injected-normals")
def _rand_injected(L, mp):
    se = _lpv_estimate(8)
    n2 = se.Σ.shape[0]
    Rn = np.random.default_rng(8).standard_normal((333, n2))
    return L.rand(L.ComplexNormal(np.asarray(se.x), se.Σ), 333, normals=Rn), L.cn_last_timing()


@case("cnormal-rand-seed-and-randn")
def _rand_seed(L, mp):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, 6))
    cn = L.ComplexNormal(np.arange(3) + 1j, A.T @ A / 6 + np.eye(6))
    return L.rand(cn, 700, seed=9), L.randn(700, 6, seed=9), L.randn(37, 13, seed=4, row0=1 << 33), L.cn_last_timing()


@case("cnormal-from-50000-samples")
def _cn_from_samples(L, mp):
    rng = np.random.default_rng(100)
    z = rng.standard_normal((50000, 3)) + 1j * rng.standard_normal((50000, 3)) @ np.array([[1.0, 0.3, 0.0], [0.0, 1.0, 0.2], [0.0, 0.0, 1.0]])
    cn = L.ComplexNormal(z)
    return cn.m, cn.Γ, cn.C


@case("cnormal-schedfunc-nMC10-phase")
def _schedfunc(L, mp):
    se = _lpv_estimate(8)
    n2 = se.Σ.shape[0]
    Rn = np.random.default_rng(10 + n2).standard_normal((10, n2))
    return L.schedfunc(se, nMC=10, phase=True, normals=Rn), L.schedfunc(se, nMC=10, phase=True, seed=11), L.cn_last_timing()


# ---- autocov / autocor (tests/test_gpu_autocov.py) -------------------------------------------------------------------------------------------
def _autocov(N, kind):
    def run(L, mp):
        rng = np.random.default_rng(N * 7 + len(kind))
        t = (100 * rng.random(N)) if kind == "random" else range(1, N + 1)
        y = rng.standard_normal(N)
        span = float(np.max(np.asarray(t, dtype=np.float64)) - np.min(np.asarray(t, dtype=np.float64)))
        out = {}
        for maxlag in ((0.5 * span, np.inf) if N <= 1000 else (0.1 * span, np.inf)):
            for fn in (L.autocov, L.autocor):
                out[f"{fn.__name__}-{maxlag}"] = fn(t, y, maxlag, normalize=True)
                out[f"{fn.__name__}-{maxlag}-timing"] = L.autofun_last_timing()
        return out
    return run


for _N in (100, 1000):
    for _kind in ("range", "random"):
        CASES[f"autocov-N{_N}-{_kind}"] = _autocov(_N, _kind)
CASES["autocov-N4097-random"] = _autocov(4097, "random")


@case("autocov-vector-of-vectors")
def _autocov_vov(L, mp):
    rng = np.random.default_rng(11)
    ts = [np.arange(30.0), 100 * rng.random(25), range(0, 40, 2), np.array([0, 1, 0, 1, 0, 1.0]), 5 * rng.random(12)]
    ys = [rng.standard_normal(len(np.asarray(t))) for t in ts]
    ys[4][:] = 2.0
    return [fn(ts, ys, maxlag, normalize=nz) for fn in (L.autocov, L.autocor) for maxlag in (np.inf, 7.5) for nz in (False, True)]


@case("autocov-count-only")
def _autocov_count(L, mp):
    from lpvspectral_jl_amd import _lib
    N = 2 ** 17
    rng = np.random.default_rng(2)
    t = np.sort(rng.random(N) * N)
    y = rng.standard_normal(N)
    off = np.array([0, N], dtype=np.int64)
    counts = []
    for kind, maxlag in ((1, np.inf), (2, 10.0)):
        n = C.c_int64(-1)
        _lib.check(_lib.lib().lpvs_autofun_f64(kind, _lib.out_ptr(t), _lib.out_ptr(y), _lib.out_ptr(off), 1, maxlag, 0, 0, None, None, 0, C.byref(n)))
        counts.append(int(n.value))
    assert counts[0] == N * (N + 1) // 2
    return counts


# ---- STFT family (tests/test_gpu_melspec.py, tests/test_gpu_welch.py) --------------------------------------------------------------------------
def _stft(n, nfft, frames, path, f32=False, nan_at=None):
    def run(L, mp):
        y = np.random.default_rng(nfft + 1).standard_normal(frames * n)
        if nan_at is not None:
            y[nan_at] = np.nan
        if f32:
            y = y.astype(np.float32)
        win = (lambda m: L.hanning(m).astype(np.float32)) if f32 else L.hanning
        out = {}
        for name, call in (("spectrogram", lambda: L.spectrogram(y, n, n // 2, nfft=nfft, window=win)),
                           ("melspectrogram", lambda: L.melspectrogram(y, n, n // 2, nfft=nfft, fs=16000, nmels=40, fmin=20, fmax=7000.0, window=win)),
                           ("mfcc", lambda: L.mfcc(y, n, n // 2, nfft=nfft, fs=16000, nmels=40, fmin=20, fmax=7000.0, nmfcc=13, window=win)),
                           ("welch_pgram", lambda: L.welch_pgram(y, n, n // 2, nfft=nfft, window=win(n))),
                           ("periodogram", lambda: L.periodogram(y[:n], nfft=nfft, window=win(n)))):
            out[name] = call()
            tm = L.stft_last_timing()
            assert tm["path"] == path and (path == 3 or tm["fft_length"] == nfft), (name, tm)
            out[name + "_timing"] = tm
        return out
    return run


CASES["stft-128-lds"] = _stft(128, 128, 20, 1)
CASES["stft-343-lds"] = _stft(343, 343, 20, 1)
CASES["stft-1009-from-1000-bluestein-lds"] = _stft(1000, 1009, 20, 3)
CASES["stft-3x2^14-four-step"] = _stft(3 * 2 ** 14, 3 * 2 ** 14, 5, 2)
CASES["stft-343-from-300-f32"] = _stft(300, 343, 5, 1, f32=True)
CASES["stft-128-one-nan"] = _stft(128, 128, 20, 1, nan_at=1234)
CASES["stft-3x2^14-one-nan"] = _stft(3 * 2 ** 14, 3 * 2 ** 14, 5, 2, nan_at=3 * 2 ** 14 + 5)


# ---- compress / heatmap (tests/test_gpu_compress.py) -------------------------------------------------------------------------------------------
@case("compress-80x50-infinities")
def _compress_inf(L, mp):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((80, 50))
    x[rng.random(x.shape) < 0.01] = np.inf
    x[rng.random(x.shape) < 0.01] = -np.inf
    y = rng.standard_normal((80, 50))
    y.ravel()[rng.permutation(4000)[:400]] = -np.inf
    return L.compress_thresholds(x, (0.1, 0.9)), L.compress_last_timing(), L.compress_thresholds(y, (0.05, 0.9)), L.compress_last_timing()


def _compress_ties(f32):
    def run(L, mp):
        x = np.round(np.random.default_rng(1).standard_normal((1000, 333)) * 4) / 4
        x = np.clip(x, -1.75, 2.0).astype(np.float32 if f32 else np.float64)                # 16 levels
        out = []
        for q in (0.005, (0.5, 0.5), (0.1, 0.9), (0, 1)):
            out += [L.compress_thresholds(x, q), L.compress_last_timing()]
            assert out[-1]["digits_skipped"] > 0
        return out
    return run


CASES["compress-ties-16-levels"] = _compress_ties(False)
CASES["compress-ties-16-levels-f32"] = _compress_ties(True)


@case("heatmap-spectrogram-128")
def _heatmap(L, mp):
    y = np.random.default_rng(129).standard_normal(20 * 128)
    return L.heatmap(L.spectrogram(y, 128, 64)), L.compress_last_timing(), L.heatmap(L.melspectrogram(y, 128, 64, fs=16000, nmels=40)), L.compress_last_timing()


# ---- uneven-record periodograms ---------------------------------------------------------------------------------------------------------------
# (tools/record_hashes.py builds its inputs with _lomb_record and _irregular and flattens results with _flat / _is_time: a change to any of
# them changes profiles/record_hashes.txt, which then has to be made again on both builds it compares)
def _lomb_record(N, ns, seed=0):                                                           # tests/test_gpu_lomb.py
    rng = np.random.default_rng(1000 * N + 10 * ns + seed)
    t = rng.integers(0, 40 * 1024, N) / 1024.0
    if N != 1000:
        t = np.sort(t)
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(ns)[None, :]) * (1.0 + np.arange(ns))[None, :] + 0.5 * rng.standard_normal((N, ns)) + 0.75
    return t, y, rng.uniform(0.5, 2.0, N)


def _irregular(Nf, lo=1):
    return np.sort(np.random.default_rng(Nf).choice(np.arange(lo, 193), Nf, replace=False)) / 64.0


def _lomb(N, ns, f, path, block=None, slabs=None):
    def run(L, mp):
        if block:
            mp.setenv("LPVS_LOMB_BLOCK", str(block))
        t, y, W = _lomb_record(N, ns)
        r = L.lombscargle(y if ns > 1 else y[:, 0], t, f(), W=W, path=path, coef=True, return_sums=True)
        tm = L.lombscargle_last_timing()
        assert tm["path"] == path and (slabs is None or tm["slabs"] == slabs) and (block is None or tm["blocks"] == (4, 4)), tm
        plain = L.lombscargle(y[:, 0], t, f(), path=path)
        return r, tm, plain
    return run


CASES["lomb-direct-N255-Nf7-ns3"] = _lomb(255, 3, lambda: _irregular(7), "direct", slabs=1)
CASES["lomb-direct-N4097-Nf65-ns3"] = _lomb(4097, 3, lambda: _irregular(65), "direct", slabs=5)
CASES["lomb-direct-N1-Nf7"] = _lomb(1, 1, lambda: _irregular(7), "direct", slabs=1)
CASES["lomb-nufft-N4097-Nf200-ns3"] = _lomb(4097, 3, lambda: (37.25 + np.arange(200)) / 64.0, "nufft")
CASES["lomb-nufft-N4097-Nf200-ns3-blocks-of-64"] = _lomb(4097, 3, lambda: (37.25 + np.arange(200)) / 64.0, "nufft", block=64)
CASES["lomb-nufft-N4097-Nf200-from-zero"] = _lomb(4097, 1, lambda: np.arange(200) / 64.0, "nufft")


def _lomb_terms(N, ns, K, slabs):                                                          # tests/test_gpu_lomb_terms.py
    def run(L, mp):
        t, y, W = _lomb_record(N, ns)
        r = L.lombscargle(y if ns > 1 else y[:, 0], t, _irregular(70, 4), W=W, coef=True, return_sums=True, nterms=K)
        tm = L.lombscargle_terms_last_timing()
        assert (tm["nterms"], tm["slabs"]) == (K, slabs), tm
        return r, tm
    return run


CASES["lomb-nterms3-N1000-ns1"] = _lomb_terms(1000, 1, 3, 1)
CASES["lomb-nterms3-N1000-ns3"] = _lomb_terms(1000, 3, 3, 1)
CASES["lomb-nterms3-N2501-ns3-three-slabs"] = _lomb_terms(2501, 3, 3, 3)


def _lomb_windows_inputs():                                                                # tests/test_gpu_lomb_windows.py: the nine explicit windows
    N, NS, SLAB = 6000, 5, 1024
    rng = np.random.default_rng(6000)
    t = np.sort(rng.integers(0, 12000 * 1024, N)) / 1024.0
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(NS)[None, :]) * (1.0 + np.arange(NS))[None, :] + 0.5 * rng.standard_normal((N, NS)) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    f = np.sort(np.random.default_rng(70).choice(np.arange(16, 193), 70, replace=False)) / 64.0
    starts = np.array([123, 5990, 1500, 100, 2900, 2000, 3000, 5743, 0], dtype=np.int64)
    counts = np.array([3 * SLAB + 5, 2, SLAB, 0, 255, SLAB + 1, 37, 257, 256], dtype=np.int64)
    last = starts + np.maximum(counts, 1) - 1
    lo, hi = t[starts] - 0.5, t[last] + 0.25
    lo[1], hi[1] = t[starts[1]], t[last[1]]
    return t, y, W, f, (starts, counts, lo, hi)


def _lomb_windows(ns, welch):
    def run(L, mp):
        t, y, W, f, wins = _lomb_windows_inputs()
        ys = y[:, :ns] if ns > 1 else y[:, 0]
        if welch:
            r = L.lombscargle_welch(ys, t, f, windows=wins, W=W, normalization="psd")
        else:
            r = L.lombscargle_spectrogram(ys, t, f, windows=wins, window=L.hanning, W=W, coef=True)
            assert list(np.flatnonzero(r[0].empty)) == [1, 3]
        tm = L.lombscargle_windows_last_timing()
        assert (tm["windows"], tm["empty"], tm["slab"], tm["items"]) == (9, 2, 1024, 12), tm
        return r, tm
    return run


CASES["lomb-spectrogram-nine-windows-ns1"] = _lomb_windows(1, False)
CASES["lomb-spectrogram-nine-windows-ns3"] = _lomb_windows(3, False)
CASES["lomb-welch-nine-windows-ns3"] = _lomb_windows(3, True)


def _boot_record(N, tone=False):                                                           # tests/test_gpu_lomb_bootstrap.py
    rng = np.random.default_rng(77 + N)
    t = np.sort(rng.integers(0, 40 * 1024, N) / 1024.0)
    y = 0.5 * rng.standard_normal(N) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    if tone:
        y = y + 0.6 * np.cos(2 * np.pi * 1.25 * t + 0.3)
    return t, y, W


def _bootstrap(budget_mb):
    def run(L, mp):
        if budget_mb:
            mp.setenv("LPVS_LOMB_BOOT_MB", budget_mb)
        t, y, W = _boot_record(301)
        r = L.lombscargle_bootstrap(y, t, _irregular(70), W=W, B=64, seed=5, return_argmax=True, return_means=True, return_power=True)
        tm = L.lombscargle_bootstrap_last_timing()
        assert tm["resamples"] == 64 and (tm["chunks"] > 1) == bool(budget_mb), tm
        return r, tm
    return run


CASES["lomb-bootstrap-B64"] = _bootstrap(None)
CASES["lomb-bootstrap-B64-in-chunks"] = _bootstrap("0.01")


@case("lomb-false-alarm-probability-bootstrap")
def _fap(L, mp):
    t, y, W = _boot_record(301, tone=True)
    f = _irregular(70)
    z = np.array([0.02, 0.05, 0.1, 0.3])
    return L.false_alarm_probability(z, y, t, f, W=W, method="bootstrap", B=64, seed=5), L.false_alarm_level(0.1, y, t, f, W=W, method="bootstrap", B=64, seed=5)


def _wwz(N, ns, c, wmin, span):                                                            # tests/test_gpu_wwz.py
    def run(L, mp):
        rng = np.random.default_rng(7000 + N)
        t = np.sort(rng.integers(0, span * 1024, N)) / 1024.0
        y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(5)[None, :]) * (1.0 + np.arange(5))[None, :] + 0.5 * rng.standard_normal((N, 5)) + 0.75
        W = rng.uniform(0.5, 2.0, N)
        f = np.sort(np.random.default_rng(70).choice(np.arange(16, 193), 70, replace=False)) / 64.0
        tau = np.rint(4 * (-0.02 * span + np.arange(9) * (1.04 * span / 8))) / 4
        r = L.wwz(y[:, :ns] if ns > 1 else y[:, 0], t, f, tau=tau, c=c, wmin=wmin, W=W, center_data=True, coef=True)
        return r, L.wwz_last_timing()
    return run


CASES["wwz-edge255-ns1"] = _wwz(255, 1, 1.0 / (128.0 * np.pi ** 2), 0.0, 64)
CASES["wwz-edge256-ns3"] = _wwz(256, 3, 1.0 / (128.0 * np.pi ** 2), 0.0, 64)
CASES["wwz-narrow-N1500-ns5-empty-cells"] = _wwz(1500, 5, 1.0 / (8.0 * np.pi ** 2), 1e-9, 375)


def _bls(N, nbins, q, ns, dips_only, center, normalization, plan):                                 # tests/test_gpu_bls.py
    def run(L, mp):
        from _bls_ref import base_case
        t, f, y = base_case(seed=0, N=N, span=64.0, Nf=70, ns=ns)
        W = 0.5 + np.random.default_rng(100 + N).random(N)
        r = L.bls(y, t, f, W=W, nbins=nbins, q=q, dips_only=dips_only, center_data=center, normalization=normalization, return_hist=True)
        tm = L.bls_last_timing()
        assert (tm["F"], tm["ts"], tm["passes"]) == plan and not tm["unit"], tm
        return r, tm
    return run


CASES["bls-n255-weights-ns3"] = _bls(255, 8, (1 / 8, 4 / 8), 3, True, False, "standard", (1, 4, 1))
CASES["bls-n257-weights-dips-and-bumps"] = _bls(257, 100, (1 / 100, 1 / 100), 1, False, True, "standard", (1, 1, 1))


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_same_bytes_whatever_the_block_held(L, monkeypatch, name):
    same_bytes_whatever_the_block_held(CASES[name], L, monkeypatch)


def test_features_interleaved_forward_and_backward(L, monkeypatch):
    """No knob at all: every case in the listed order, then in reverse, in one process -- each call of the second pass takes blocks that other
    features left behind.  The same bytes both times."""
    forward = {name: _run(fn, L, monkeypatch, None) for name, fn in CASES.items()}
    bad = []
    for name in reversed(list(CASES)):
        d = _differences(forward[name], _run(CASES[name], L, monkeypatch, None))
        if d:
            bad.append(f"{name}: " + "; ".join(d[:4]))
        del forward[name]
    assert not bad, "\n".join(bad)
