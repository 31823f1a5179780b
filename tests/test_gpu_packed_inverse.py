"""The packed inverse of every storage, read back ENTRY BY ENTRY through unit mat-vecs and compared with its host model
(tests/_packed_ref.py, written from DESIGN.md 4.1), for every kernel that streams it.  GPU only.

A handle built from a zero record has b = 0 and therefore xb = 0 exactly; `admm_set_state(x = 0, z = mu s e_j, u = 0, iters = k)`
followed by ONE iteration leaves x = M~ (z - u)/mu = s M~[:, j].  mu and s are powers of two, so the right-hand side is exactly
s e_j and every product s m~ is exact: the kernels that store tile partials (two launches per iteration, the MFMA kernel of
several signals, the full-matrix kernels of n < 2048) add one non-zero per row and must return the model BIT FOR BIT; the one-launch
iteration rounds each row once to its quantum q (rule in the header of csrc/admm_one_launch.hip, restated in
_packed_ref.one_launch_quantum) and must be within q/2 plus one ulp.  k = 0 and k = 1 take the two tile orders of the mirrored
schedule.  Handles that read 32 of the 36 bits are held to the 32-bit model at launches after which no refresh of the stale nibble
product is due (17 and 34), and at launches 0 and 1, whose refresh is committed before their x is formed, to the 36-bit model, with the
nibble term taken from the offset vector equal to N rhs.  The bytes `time_matvec` reports must be those of the model's per-tile format map.

Dense right-hand sides (Gaussian, 12 decades, one block, alternating signs) on the same handles -- every signal slot of a
several-signal handle its own -- are held componentwise to
gamma_(np+4) (|M~| |v|) -- np products and sums per row in any order, the gather, the offset add, the integer-to-double conversion
and the reference's own rounding -- plus, for the one-launch iteration, (row blocks) q/2: every tile that touches a row adds one
rounded addend, np/128 of them.

Window batches have no state entry per column (no set_state on a batch): they stay out of scope here.
"""
import numpy as np
import pytest

import _packed_ref as R
from _guards import precondition_not_met

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
PROBES = ((0, 8.0), (1, -2.0 ** -5))               # (iteration index = tile-order parity, s)
# Handles that read 32 bits refresh the stale nibble product after every launch up to 15, every 2nd up to 31, every 4th up to 63, ...
# (nib_refresh_due), and a refresh is committed to the offset vector BEFORE the x of its launch is formed: the x of a launch that is due
# carries all 36 bits, xb_corr + N rhs + M32 rhs.  Launches 34 and 17 are not due (one of each parity): they show the 32-bit reads alone.
PROBES32 = ((0, 8.0, True), (1, -2.0 ** -5, True), (34, 8.0, False), (17, -2.0 ** -5, False))
SHAPES = {130: (13, 5, 1 << 14), 1000: (125, 4, 1 << 14), 2048: (128, 8, 1 << 18), 2304: (144, 8, 1 << 18), 2096: (131, 8, 1 << 18),
          8192: (512, 8, 1 << 20)}               # n = 2 Nf Nv: (Nf, Nv, samples) -- enough samples for a diagonally dominant inverse
COUNTS = {}                                        # (storage, kernel) -> [entries compared, ties met, worst dense ratio], printed when the module ends


def _signal(N, Nf, rng):
    X = np.sort(rng.random(N) * (10.0 * N / 500)); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
    return X, V, w


def _lpv(L, n, ns=1, f32=False):
    Nf, Nv, N = SHAPES[n]
    X, V, w = _signal(N, Nf, np.random.default_rng(n))
    if f32:
        X, V, w = (a.astype(np.float32) for a in (X, V, w))
    dt = np.float32 if f32 else np.float64
    if ns > 1:
        return L.Problem.lpv_multi(np.zeros((N, ns), dtype=dt, order="F"), X, V, w, Nv)
    return L.Problem.lpv(np.zeros(N, dtype=dt), X, V, w, Nv)


def _wide_gram(n):
    """The wide-range matrix of test_gpu_split_storage.py: a diagonally dominant SPD matrix whose inverse spans ~12 decades."""
    rng = np.random.default_rng(7)
    B = rng.standard_normal((n, 8)) * 1e-2
    return np.diag(np.logspace(-3, 3, n)) + B @ B.T


def _block_gram(n, blocks=4):
    """Block-diagonal: the inverse has whole tiles of exact zeros."""
    rng = np.random.default_rng(8)
    G = np.zeros((n, n))
    m = n // blocks
    for q in range(blocks):
        C = rng.standard_normal((m, 24))
        G[q * m:(q + 1) * m, q * m:(q + 1) * m] = np.diag(1.0 + 50.0 * rng.random(m)) + 0.02 * (C @ C.T)
    return G


def _init(L, p, mu, storage=None, iteration=None, nt_loads=None, xcorr="off"):
    p.set_option("storage", storage)
    p.set_option("iteration", iteration)
    p.set_option("nt_loads", nt_loads)
    p.set_option("xupdate_correction", xcorr)
    p.set_prox(L.NormL1(1.0))
    p.admm_init(None, μ=mu, tol=0.0)
    return p.matvec_info()


def _state(p, cols, mu, s):
    dt = np.float32 if p.f32 else np.float64
    z = np.zeros((p.n, p.ns), dtype=dt, order="F")
    for q, j in enumerate(cols):
        z[j, q] = mu * s
    return z if p.ns > 1 else z[:, 0]


def _read_columns(p, mu, s, k, want_nibble=False):
    """x of one iteration from the state (0, mu s e_j, 0) at iteration index k, for every j: n x n; the nibble term of the offset vector too."""
    n, ns = p.n, p.ns
    X = np.empty((n, n))
    Nb = np.empty((n, n)) if want_nibble else None
    zero = np.zeros((n, ns) if ns > 1 else n, dtype=np.float32 if p.f32 else np.float64, order="F")
    for j0 in range(0, n, ns):
        cols = list(range(j0, min(j0 + ns, n)))
        # (a corrected handle re-entered at k > 0 corrects its offset vector from the state handed in: the zero one is put back)
        p.admm_set_state(zero, _state(p, cols, mu, s), zero, iters=k, offset=np.zeros(2 * n) if want_nibble and k > 0 else None)
        it, _, _ = p.admm_run(1)
        assert it == k + 1
        x = p.admm_get(f64=True)[0]
        X[:, cols] = (x if ns > 1 else x[:, None])[:, :len(cols)]
        if want_nibble:
            off = p.admm_get_offset()
            assert off.size == 2 * n
            Nb[:, j0] = off[:n] - off[n:]
    return X, Nb


def _mismatch(X, ref, tol=None):
    bad = (X != ref) if tol is None else ~(np.abs(X - ref) <= tol)
    if not bad.any():
        return None
    i, j = np.argwhere(bad)[0]
    return (f"{int(bad.sum())} of {bad.size} entries differ; first at row {i} (block {i // 128}), column {j} (block {j // 128}): "
            f"read {X[i, j]!r}, model {ref[i, j]!r}, |diff| max {np.nanmax(np.abs(X - ref)):.3e}")


def _dense_vectors(n, rng):
    v = [rng.standard_normal(n), rng.standard_normal(n) * 1e3,
         rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n), rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 0, n)]
    for lo in (0, (n // 128 - 1) * 128 if n >= 256 else n // 2):
        b = np.zeros(n); b[lo:lo + 128] = rng.standard_normal(min(128, n - lo)); v.append(b)
    v += [np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + rng.random(n)), np.where(np.arange(n) % 2 == 0, 1.0, -1.0)]
    return [a.astype(np.float32).astype(np.float64) for a in v]          # (representable in the I/O type of _f32 handles too)


def _check_dense(p, A, parts, mu, one_launch, label, ks=(0, 1)):
    """Eight dense right-hand sides per signal slot (slot q of pass i takes vector i + q: every slot its own) on both parities
    (launch indices `ks`) against M~ v in long double; returns the largest error / bound.  `parts`: the matrices whose products make
    up x -- (M~,), or (M32, N) at a launch whose nibble refresh is due: each product is within gamma of its own |.||v|, and the
    one-launch iteration rounds each of them once per tile."""
    n, ns = p.n, p.ns
    np_ = R.padded_size(n)
    rng = np.random.default_rng(n + 17)
    Ml = sum(m.astype(np.longdouble) for m in parts)
    Mabs = sum(np.abs(m) for m in parts)
    gam = (np_ + 4) * U / (1 - (np_ + 4) * U)
    dt = np.float32 if p.f32 else np.float64
    zero = np.zeros((n, ns) if ns > 1 else n, dtype=dt, order="F")
    vecs = _dense_vectors(n, rng)
    worst = 0.0
    for idx in range(len(vecs)):
        V = np.stack([vecs[(idx + q) % len(vecs)] for q in range(ns)], axis=1)
        ref = Ml @ V.astype(np.longdouble)
        bound = gam * (Mabs @ np.abs(V))
        if one_launch:
            bound = bound + len(parts) * (np_ // 128) * R.one_launch_quantum(A, n, float(np.abs(V).max())) / 2
        for k in ks:
            z = np.asfortranarray((mu * V).astype(dt))
            assert np.array_equal(z.astype(np.float64) / mu, V)
            p.admm_set_state(zero, z if ns > 1 else z[:, 0], zero, iters=k, offset=np.zeros(2 * n) if p._offset_len() == 2 * n and k > 0 else None)
            p.admm_run(1)
            x = p.admm_get(f64=True)[0].reshape(n, ns, order="F")
            err = np.abs((x.astype(np.longdouble) - ref).astype(np.float64))
            assert np.all(err[bound == 0] == 0), (label, idx, k)
            r = float((err[bound > 0] / bound[bound > 0]).max())
            worst = max(worst, r)
            assert r <= 1.0, (label, "rhs", idx, "launch", k, "error / bound", r)
    return worst


def _storage_key(p, storage, xcorr):
    if p.f32:
        return "f32"
    if storage in (None, "mixed32"):
        return "mixed32" if (xcorr != "off" and p.ns == 1) else "mixed"
    return storage


def _expected_kernel(p, eff, iteration):
    """(kernel, one launch per iteration) for the storage in effect `eff` ("full": n < 2048)."""
    if eff == "full":
        return ("admm_small_iter_kernel", True) if iteration != "two" and p.ns == 1 else ("symv_kernel", False)
    if p.ns > 1:
        return "symv_tile_mfma_ws_kernel", False
    if eff in ("mixed", "mixed32"):
        return ("admm_iter_mixed_kernel", True) if iteration != "two" else ("symv_tile_mixed_kernel", False)
    if eff == "f32":
        return ("admm_iter_mixed_kernel", True) if iteration != "two" else ("symv_tile_f32_kernel", False)
    return {"split": "symv_tile_split_kernel", "f64": "symv_tile_kernel<double>"}[eff], False


def _run_case(L, p, A, mu, storage=None, iteration=None, nt_loads=None, xcorr="off", dense=True, want=None):
    """One handle configuration: kernel and bytes as the model says, every entry of M~ on both parities, the dense products."""
    n, ns = p.n, p.ns
    info = _init(L, p, mu, storage, iteration, nt_loads, xcorr)
    key = _storage_key(p, storage, xcorr)
    model = R.packed_model(A, n, ns=ns, storage=key)
    eff = model["storage"]
    if want is not None and eff != want:
        precondition_not_met(f"this case is about the {want} storage, the model of this inverse says {eff}")
    kernel, one = _expected_kernel(p, eff, iteration)
    label = f"n={n} ns={ns} storage={eff} kernel={kernel} iteration={'one' if one else 'two'} nt={nt_loads}"
    assert info["kernel"] == kernel and bool(info.get("one_launch_iteration", False)) == one, (label, info)
    one = one and kernel == "admm_iter_mixed_kernel"      # (the one-launch kernel of n < 2048 stores doubles: no quantum, exact)
    if eff in ("mixed", "mixed32"):
        assert ("32 leading bits" in info["storage"]) == (eff == "mixed32"), (label, info)
    assert p.time_matvec(1)[1] == model["bytes"], (label, p.time_matvec(1)[1], model["bytes"])
    Mread = model["M32"] if eff == "mixed32" else model["Mt"]
    probes = PROBES32 if eff == "mixed32" else tuple(pr + (None,) for pr in PROBES)
    for k, s, due in probes:
        X, Nb = _read_columns(p, mu, s, k, want_nibble=eff == "mixed32")
        ref = s * (model["Mt"] if due else Mread)                      # (a due launch: 32-bit reads + the nibble term = the 36-bit matrix)
        nref = None if Nb is None else (s * model["N"] if due else np.zeros((n, n)))
        if one:
            q = R.one_launch_quantum(A, n, abs(s))                     # (a due launch rounds twice: the product and the nibble product)
            msg = _mismatch(X, ref, (q if due else q / 2) + np.spacing(np.abs(ref)))
            assert msg is None, (label, "launch", k, "quantum", q, msg)
            if Nb is not None:
                msg = _mismatch(Nb, nref, q / 2 + np.spacing(np.abs(nref)) if due else None)
                assert msg is None, (label, "nibble term, launch", k, msg)
        else:
            msg = _mismatch(X, ref)
            assert msg is None, (label, "launch", k, msg)
            if Nb is not None:
                msg = _mismatch(Nb, nref)
                assert msg is None, (label, "nibble term, launch", k, msg)
    types = model["types"]
    ties = 0
    if eff == "split" or types is not None:
        tmask = R.split_ties(R.pad_device(A, n, R.padded_size(n)))
        for t, (I, J) in enumerate(R.tile_list(R.padded_size(n))):
            if eff == "split" or types[t] == R.FLOAT_HEAD:
                ties += int(tmask[I * 128:(I + 1) * 128, J * 128:(J + 1) * 128].sum())
    c = COUNTS.setdefault((eff, kernel), [0, 0, 0.0])
    c[0] += len(probes) * n * n
    c[1] += ties
    worst = 0.0
    if dense and eff == "mixed32":                         # launches that are not due: the 32-bit reads; due: + the nibble product
        worst = max(_check_dense(p, A, (Mread,), mu, one, label, ks=(34, 17)), _check_dense(p, A, (Mread, model["N"]), mu, one, label, ks=(0, 1)))
    elif dense:
        worst = _check_dense(p, A, (Mread,), mu, one, label)
    c[2] = max(c[2], worst)
    fmt = "" if types is None else f" tiles float-head/fixed/fixed-diagonal {int((types == 0).sum())}/{int((types == 1).sum())}/{int((types == 2).sum())}"
    print(f"[packed-inverse] {label}: {len(probes) * n * n} entries, {ties} ties in float-head tiles, {model['bytes']} B,{fmt} worst dense ratio {worst:.3f}")
    model["info"] = info
    return model


@pytest.fixture(scope="module")
def handles(L):
    """Problems (zero record) and their inverses, built once per (kind, n, ns, f32, mu)."""
    cache = {}

    def get(kind, n, mu, ns=1, f32=False):
        key = (kind, n, mu, ns, f32)
        if key not in cache:
            if kind == "lpv":
                p = _lpv(L, n, ns, f32)
            elif kind == "wide":
                p = L.Problem.gram(_wide_gram(n), np.zeros(n))
            else:
                p = L.Problem.gram(_block_gram(n), np.zeros(n))
            assert not np.any(p.get_rhs()), "a zero record must give b = 0"
            A = np.ascontiguousarray(p.get_inverse(1.0 / mu).T)          # device row-major: A[r, c] = M[r][c]; first: it clears `inited`
            cache[key] = (p, A)
        return cache[key]
    yield get
    for p, _ in cache.values():
        p.close()
    for (eff, kernel), (entries, ties, worst) in sorted(COUNTS.items()):       # the totals DESIGN 6 quotes
        print(f"[packed-inverse total] storage {eff:8s} kernel {kernel:28s}: {entries} entries compared, {ties} ties in float-head tiles, worst dense ratio {worst:.3f}")


CONFIGS = [("default", dict(xcorr="on"), "mixed32"), ("default-two", dict(xcorr="on", iteration="two"), "mixed32"),
           ("mixed", dict(storage="mixed"), "mixed"), ("mixed-nt-on", dict(storage="mixed", nt_loads="on"), "mixed"),
           ("mixed-nt-off", dict(storage="mixed", nt_loads="off"), "mixed"), ("mixed-two", dict(storage="mixed", iteration="two"), "mixed"),
           ("split", dict(storage="split"), "split"), ("f64", dict(storage="f64"), "f64")]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("n", [2048, 2304, 2096])
def test_every_entry_of_the_packed_inverse_lpv(L, handles, n, cfg):
    mu = 2.0 ** -4
    p, A = handles("lpv", n, mu)
    m = _run_case(L, p, A, mu, want=cfg[2], **cfg[1])     # (n = 2096 too: pad rows inside fixed-point tiles are read out, not a fall-back)
    if cfg[0] == "mixed":                                  # both tile formats in the same matrix: float-head diagonal tiles, fixed point below
        assert (m["types"] == R.FLOAT_HEAD).any() and (m["types"] != R.FLOAT_HEAD).any(), m["types"]


@pytest.mark.parametrize("iteration", ["one", "two"])
@pytest.mark.parametrize("n", [2048, 2304, 2096])
def test_every_entry_of_the_packed_inverse_f32_handles(L, handles, n, iteration):
    mu = 2.0 ** -4
    p, A = handles("lpv", n, mu, f32=True)
    _run_case(L, p, A, mu, iteration=iteration, want="f32")


@pytest.mark.parametrize("iteration", ["one", "two"])
@pytest.mark.parametrize("n", [130, 1000])
def test_every_entry_of_the_full_matrix_kernels(L, handles, n, iteration):
    p, A = handles("lpv", n, 2.0 ** -4)
    _run_case(L, p, A, 2.0 ** -4, iteration=iteration, want="full")


@pytest.mark.parametrize("cfg", [("default", dict(xcorr="on")), ("mixed", dict(storage="mixed"))], ids=["default", "mixed"])
def test_forward_tile_order_reads_the_same_matrix(L, handles, cfg, monkeypatch):
    monkeypatch.setenv("LPVS_TILE_ORDER", "forward")
    p, A = handles("lpv", 2304, 2.0 ** -4)
    _run_case(L, p, A, 2.0 ** -4, **cfg[1])


@pytest.mark.parametrize("cfg", [("default", dict(xcorr="on")), ("f32", dict())], ids=["default", "f32"])
def test_every_entry_of_the_packed_inverse_at_8192(L, handles, cfg):
    p, A = handles("lpv", 8192, 2.0 ** -4, f32=cfg[0] == "f32")
    _run_case(L, p, A, 2.0 ** -4, want="mixed32" if cfg[0] == "default" else "f32", **cfg[1])


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[0] in ("default", "default-two", "mixed", "mixed-two", "split", "f64")], ids=lambda c: c[0])
@pytest.mark.parametrize("kind,n", [("wide", 2048), ("wide", 2000), ("block", 2048)])
def test_every_entry_of_the_packed_inverse_explicit_grams(L, handles, kind, n, cfg):
    """Entries over ~12 decades (mu = 1), a padded size, and whole tiles of exact zeros."""
    p, A = handles(kind, n, 1.0)
    m = _run_case(L, p, A, 1.0, want=cfg[2] if n == 2048 or cfg[2] in ("split", "f64") else None, **cfg[1])
    if kind == "block":
        assert np.count_nonzero(A[:512, 512:]) == 0 and np.count_nonzero(m["Mt"][:512, 512:]) == 0


@pytest.mark.parametrize("mfma16", [False, True], ids=["q4", "mfma16"])
@pytest.mark.parametrize("storage", ["f64", "split", "mixed"])
@pytest.mark.parametrize("ns", [3, 8, 12])
def test_every_entry_of_the_packed_inverse_several_signals(L, handles, ns, storage, mfma16, monkeypatch):
    if mfma16:
        monkeypatch.setenv("LPVS_MULTI_MFMA", "16")
    else:
        monkeypatch.delenv("LPVS_MULTI_MFMA", raising=False)
    p, A = handles("lpv", 2048, 2.0 ** -4, ns=ns)
    m = _run_case(L, p, A, 2.0 ** -4, storage=storage, want=storage)
    assert m["info"]["signals_per_pass"] == (16 if mfma16 or ns > 8 else 8), m["info"]


def test_fixed_point_tiles_keep_the_promise_of_the_admission_rule(L, handles):
    """every fixed-point tile's steps are <= 2^-44 max|M[:n, :n]| sqrt(8192/np).  Padded problems carry ones on the pad
    diagonal of M; counted into max|M| they would loosen the rule by 1/mu.  n = 2096 at mu = 2^-10 (80 pad rows) and a Fourier handle
    with a zero frequency (n = 2 Nf - 1).  Two assertions bind the device: the bytes it streams are those of the model's map under the
    rule over the valid rows (the map under the rule over all np rows has other bytes in at least one case, or the test is red), and
    the read-out of every entry equals that model -- a tile admitted against the rule would read back in the other format."""
    rng = np.random.default_rng(5)
    Nf, N = 1100, 1 << 16
    t = np.sort(rng.random(N) * N)
    f = np.arange(Nf) / (2.2 * Nf)
    cases = [("lpv n=2096", ) + handles("lpv", 2096, 2.0 ** -10) + (2.0 ** -10,)]
    pf = L.Problem.fourier(np.zeros(N), t, f)
    try:
        assert pf.n == 2 * Nf - 1
        Af = np.ascontiguousarray(pf.get_inverse(2.0 ** 10).T)
        cases.append(("fourier n=2199", pf, Af, 2.0 ** -10))
        discriminates = False
        for name, p, A, mu in cases:
            n = p.n
            valid, padded = R.packed_model(A, n, storage="mixed", absmax="valid"), R.packed_model(A, n, storage="mixed", absmax="padded")
            info = _init(L, p, mu, "mixed")
            nbytes = p.time_matvec(1)[1]
            print(f"[pad-diagonal] {name}: max|M| valid {valid['absmax']:.3e}, with the pad 1.0; limit {valid['limit']:.3e}; fixed tiles under the rule over "
                  f"valid rows {int(np.count_nonzero(valid['types']))} ({valid['bytes']} B), over all np rows {int(np.count_nonzero(padded['types']))} "
                  f"({padded['bytes']} B); the device streams {nbytes:.0f} B")
            assert nbytes == valid["bytes"], (name, "device bytes", nbytes, "rule over the valid rows", valid["bytes"], "over np rows", padded["bytes"])
            kernel, one = _expected_kernel(p, valid["storage"], None)
            assert info["kernel"] == kernel, (name, info)
            X, _ = _read_columns(p, mu, 1.0, 0)
            q = R.one_launch_quantum(A, n, 1.0)
            msg = _mismatch(X, valid["Mt"], q / 2 + np.spacing(np.abs(valid["Mt"])) if one else None)
            assert msg is None, (name, msg)
            discriminates = discriminates or padded["bytes"] != valid["bytes"]
        if not discriminates:
            precondition_not_met("neither case has a tile between the two limits: the test would not see the pad diagonal in max|M|")
    finally:
        pf.close()


# ---- _f32 handles: 300 iterations against the exact model of their own arithmetic -----------------------------------------------
def _f32_problem(n, seed):
    Nf, Nv = n // 16, 8
    rng = np.random.default_rng(seed)
    N = 5000
    X = np.sort(rng.random(N) * 10 * N / 500).astype(np.float32)
    V = np.linspace(0, 1, N).astype(np.float32)
    w = (2 * np.pi * (np.arange(Nf) + 1.0) * 25 / Nf / 4).astype(np.float32)
    y = (2 * V ** 2 * np.cos(w[12] * X) + 2 / (5 * V + 1) * np.cos(w[60] * X) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return y, X, V, w, Nf, Nv


@pytest.mark.parametrize("kind", ["group", "l1", "l0", "ball"])
@pytest.mark.parametrize("n", [2048, 2096])
def test_f32_iterates_against_the_model_of_their_own_storage(L, oracle, n, kind):
    """The _f32 storage is held to 2e-5 of the f64 oracle elsewhere -- the distance of fl32(M) from M, which hides everything below
    it.  Against the ADMM carried in extended precision WITH M~ = fl32(M) and the handle's own offset vector (oracle
    lpvo_admm_minv_ld) only the f64 arithmetic of the iteration is left, the same as the f64 path's: the project's parity bound of
    tests/test_gpu_parity.py applies, rel-L2 <= 1e-9 in x, z, u with identical support, after 300 iterations, both launch schemes.
    Measured (MI355X): see DESIGN.md 6."""
    mu, iters = 0.05, 300
    y, X, V, w, Nf, Nv = _f32_problem(n, 21 + n)
    prox, oprox = {"group": (L.SlicedSeparableSum.frequency_groups(3.0, Nf, 2 * Nv), oracle.GroupL2(3.0, 2 * Nv)),
                   "l1": (L.NormL1(1.0), oracle.NormL1(1.0)), "l0": (L.NormL0(1.0), oracle.NormL0(1.0)),
                   "ball": (L.IndBallL0(20), oracle.IndBallL0(20))}[kind]
    with L.Problem.lpv(y, X, V, w, Nv) as p:
        assert p.f32 and p.n == n
        A = np.ascontiguousarray(p.get_inverse(1.0 / mu).T)
        Mt = R.packed_model(A, n, storage="f32")["Mt"]
        ref = None
        for iteration in ("one", "two"):
            p.set_option("iteration", iteration)
            p.set_option("xupdate_correction", "off")
            p.set_prox(prox)
            p.admm_init(None, μ=mu, tol=0.0)
            info = p.matvec_info()
            fusable = kind != "ball"
            assert info["kernel"] == ("admm_iter_mixed_kernel" if iteration == "one" and fusable else "symv_tile_f32_kernel"), info
            xb = p.admm_get_offset()
            assert xb is not None and xb.size == n and np.any(xb)
            if ref is None:
                ref = oracle.admm_minv_ld(Mt, xb, oprox, [iters], mu=mu)[iters]
            it, _, _ = p.admm_run(iters)
            assert it == iters
            got = p.admm_get(f64=True)
            d = [float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300)) for g, r in zip(got, ref)]
            print(f"[f32-model] n={n} {kind} iteration={iteration} ({info['kernel']}): rel-L2 to the fl32(M) model x {d[0]:.2e} z {d[1]:.2e} u {d[2]:.2e}")
            assert max(d) <= 1e-9, (n, kind, iteration, d)
            assert np.array_equal(got[1] != 0, ref[1] != 0), (n, kind, iteration)
