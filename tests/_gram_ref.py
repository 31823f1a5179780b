"""Shared by tests/test_gram_ref_host.py and tests/test_gpu_gram_dense.py: the cases that reach every instance of the dense Gram kernel
(csrc/gram.hip), their inputs, the host mirror of the tile / chunk plan and the entrywise bound.

The bound.  A sum of N products evaluated in doubles in ANY order (MFMA 4-sample steps, 32-sample stages, sample chunks summed in fixed order,
four fma chains per right-hand-side block ...) satisfies |fl(sum) - sum| <= gamma_N sum|terms| ~ N u sum|terms|, u = 2^-53.  The operands the
kernels multiply are not the entries of Phi but roundings of the same real numbers: KR forms T K per operand (one rounding each: (1+u)^2 per
term), KRS forms T' (K_j K_j') (two roundings against the two of Phi_a Phi_b: <= 3 ulp per term as gram.hip says), the weighted panel form
rounds W P once, the right-hand sides round W y once; that is at most 4 u per term against the product of the entries of Phi, and 16 u covers it
four times over.  Hence, per entry and with S = sum_k |W_k Phi_ka Phi_kb| from the long-double reference,

    |G - G_ref| <= (N + 16) 2^-53 S        |b - b_ref| <= (N + 16) 2^-53 s .

No entry is exempt and no maximum over the matrix is taken."""
import numpy as np

U = 2.0 ** -53
TM, TN, BK_ALIGN = 128, 256, 64          # csrc/gram.hip


def bound(N, S):
    return (N + 16) * U * S


def worst_ratio(got, ref, N, S):
    """max over entries of |got - ref| / bound; S > 0 is the caller's precondition."""
    return float(np.max(np.abs(got - ref) / bound(N, S)))


# ---- host mirror of the plan (gram.hip: make_tiles, make_tiles_pairs, choose_split) -------------------------------------------
def tiles_lower(n):
    nti = -(-n // TM)
    return [(ti, tj) for ti in range(nti) for tj in range(ti // 2 + 1)]


def tiles_pairs(np2, P):
    nti, ntj = -(-np2 // TM), -(-(np2 * P) // TN)
    out = []
    for ti in range(nti):
        plast = min(ti * TM + TM - 1, np2 - 1)
        out += [(ti, tj) for tj in range(ntj) if (tj * TN) // P <= plast]
    return out


def choose_split(tiles, N, nbatch=1):
    """-> (ksplit, rows_per_chunk)"""
    nstage = -(-N // BK_ALIGN)
    max_split = max(nstage // 8, 1)
    want = min(-(-256 * 16 // (tiles * nbatch)), max_split)
    best, best_eff = 1, -1.0
    for ks in range(max(want // 2, 1), min(want * 2, max_split) + 1):
        items = tiles * ks * nbatch
        eff = items / (-(-items // 256) * 256)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, ks
    rpc = -(-(-(-N // best)) // BK_ALIGN) * BK_ALIGN
    return best, rpc


def plan(form, n, N, Nf=0, nb=0):
    """What the handle must report: tiles, tile columns, ksplit, rows per chunk, issued flops."""
    tl = tiles_pairs(2 * Nf, nb * (nb + 1) // 2) if form == "krs" else tiles_lower(n)
    ks, rpc = choose_split(len(tl), N)
    return dict(tiles=len(tl), tile_rows=len({t[0] for t in tl}), tile_cols=len({t[1] for t in tl}), ksplit=ks, rows_per_chunk=rpc,
                issued=len(tl) * 128.0 * 256.0 * 2.0 * (ks * rpc))


# ---- the LPV cases: (id, Nf, Nv, N, option gram_form, form that must run, samples per stage, normalize, half-width of V) -------------
# KRS: nb <= 18 -> gram_kernel<2,32>, nb = 19 .. 31 -> gram_kernel<2,16>; nb >= 32: the pair table no longer fits -> KR.
# KR:  gram_kernel<0,32> unless two 32-sample images exceed 160 KiB: nb = 1 (65 + 129 frequencies per tile) and nb >= 312 (the
#      activation rows) -> <0,16>; nb >= 632 -> <0,8>.
LPV_CASES = [
    ("krs-70x2", 70, 2, 1500, None, "krs", 32, True, 1.0),          # P = 3; G3 140 rows: second tile row of 12; nq = 420: partial second tile column; clamps
    ("krs-70x2-N333", 70, 2, 333, None, "krs", 32, True, 1.0),      # one chunk, 51 pad rows
    ("krs-66x5", 66, 5, 1500, None, "krs", 32, False, 1.0),         # P = 15, 2 nb does not divide 128; band tiles with skipped waves; normalize = false
    ("krs-66x8", 66, 8, 1500, None, "krs", 32, True, 1.0),          # the benchmark's nb at a size with partial tiles
    ("krs-8x20", 8, 20, 1500, None, "krs", 16, True, 1.0),          # gram_kernel<2,16>: one tile row x 14 columns
    ("krs-65x19", 65, 19, 1500, None, "krs", 16, True, 1.0),        # gram_kernel<2,16>: two tile rows
    ("krs-6x31", 6, 31, 1500, None, "krs", 16, True, 1.0),          # last nb the pair form fits (P = 496)
    ("kr-auto-5x32", 5, 32, 1500, None, "kr", 32, True, 1.0),       # KRS no longer fits: hand-over to KR, ldk > 32
    ("kr-auto-3x50", 3, 50, 1500, None, "kr", 32, True, 1.0),
    ("kr-150x1", 150, 1, 1500, "kr", "kr", 16, True, 1.0),          # gram_kernel<0,16>
    ("kr-150x1-as-krs", 150, 1, 1500, "krs", "kr", 16, True, 1.0),  # gram_krs_fits needs nb >= 2: asking for krs runs kr
    ("kr-50x3", 50, 3, 1500, "kr", "kr", 32, False, 1.0),           # a frequency straddles the 128- and 256-column tile edges; normalize = false
    ("kr-22x7", 22, 7, 1500, "kr", "kr", 32, True, 1.0),            # the same, masked columns beyond n
    ("kr-22x7-N333", 22, 7, 333, "kr", "kr", 32, True, 1.0),
    ("kr-20x8", 20, 8, 1500, "kr", "kr", 32, True, 1.0),            # the one_k shortcut (2 nb == 16), partial last tile
    ("kr-17x8", 17, 8, 1500, "kr", "kr", 32, True, 1.0),
    ("krs-20x8", 20, 8, 1500, "krs", "krs", 32, True, 1.0),         # the same two shapes through KRS: the one_k results must sit inside the same bound
    ("krs-17x8", 17, 8, 1500, "krs", "krs", 32, True, 1.0),
    ("kr-1x320", 1, 320, 1500, "kr", "kr", 16, True, 0.1),          # gram_kernel<0,16> through the activation rows
    ("kr-1x640", 1, 640, 1500, "kr", "kr", 8, True, 0.1),           # gram_kernel<0,8>
]
LPV_IDS = [c[0] for c in LPV_CASES]


def lpv_inputs(case, ns=1):
    """Non-uniform sorted grid (nowhere near an arithmetic progression), unsorted X and V with both signs."""
    cid, Nf, Nv, N = case[:4]
    rng = np.random.default_rng(1000 * Nf + 7 * Nv + N)
    X = rng.uniform(-3.0, 5.0, N)
    V = rng.uniform(-case[8], case[8], N)
    w = np.sort(rng.uniform(0.4, 6.0, Nf))
    Y = rng.standard_normal((N, ns))
    return (Y[:, 0] if ns == 1 else Y), X, V, w


# ---- the Fourier (PANEL) cases: (id, Nf, zero frequency, weights, N) -----------------------------------------------------------------
FOURIER_CASES = [
    ("panel-340", 170, False, False, 1500),        # two tile columns, ld = 512
    ("panel-340-W", 170, False, True, 1500),       # weights on the A operand only, zero pad weights
    ("panel-339", 170, True, False, 1500),         # odd n
    ("panel-339-W", 170, True, True, 1500),
    ("panel-339-W-N333", 170, True, True, 333),
]
FOURIER_IDS = [c[0] for c in FOURIER_CASES]


def fourier_inputs(case):
    cid, Nf, zero, weighted, N = case
    rng = np.random.default_rng(50000 + 2 * Nf + int(zero) + 10 * int(weighted) + N)
    t = np.cumsum(0.5 + rng.random(N))
    f = np.sort(rng.uniform(0.01, 0.45, Nf))
    if zero:
        f[0] = 0.0
    y = rng.standard_normal(N)
    W = 0.1 + rng.random(N) if weighted else None
    return y, t, f, W


def integer_family(N, n=300, seed=3):
    rng = np.random.default_rng(seed + N)
    return rng.integers(-3, 4, (N, n)).astype(np.float64), rng.integers(-2, 3, N).astype(np.float64)


# ---- the structured forms (ap, ap-nufft) at pair scale -------------------------------------------------------------------------------
# They turn products of trig values into sums (cos a cos b = (cos(a-b) + cos(a+b)) / 2), so an entry is not bounded by S[a][b]: the terms
# cancel.  Their natural scale is the weight sum of the activation pair, C[j][j'] = sum_k |K_kj K_kj'| (Fourier: sum_k |W_k| / (2 Nf), the
# weights times the regressor's 1/sqrt(2 Nf) twice), and the project's stated tolerance is 1e-12 plus the phase term
# 4.5e-16 max|w| max|x|, applied here per pair instead of to max|G|.
STRUCT_LPV_CASES = [("ap-24x3", 24, 3, 4096), ("ap-20x8", 20, 8, 4096)]
STRUCT_FOURIER_CASES = [("ap-fourier", 40, False, False, 5000), ("ap-fourier-zero", 40, True, False, 5000),
                        ("ap-fourier-W", 40, False, True, 5000), ("ap-fourier-zero-W", 40, True, True, 5000)]


def struct_tol(wmax, xmax):
    return 1e-12 + 4.5e-16 * wmax * xmax


def struct_lpv_inputs(case):
    cid, Nf, Nv, N = case
    rng = np.random.default_rng(900 + Nf + Nv)
    X = rng.permutation(np.sort(rng.random(N)) * 50.0)
    V = rng.uniform(-1.0, 1.0, N)
    w = 2 * np.pi * np.arange(1, Nf + 1) / 7.0                   # an arithmetic progression
    return rng.standard_normal(N), X, V, w


def struct_fourier_inputs(case):
    cid, Nf, zero, weighted, N = case
    rng = np.random.default_rng(17 + int(zero) + 2 * int(weighted))
    t = np.sort(rng.random(N) * 300.0)
    f = (np.arange(Nf) if zero else np.arange(1, Nf + 1)) / 97.0
    y = np.sin(2 * np.pi * f[7] * t) + 0.2 * rng.standard_normal(N)
    return y, t, f, (rng.random(N) + 0.5 if weighted else None)


# ---- the structured forms where the low words of their phases decide (tests/_phase_ref.py holds the reference) -----------------------------
# u = 2^-53.  Bound per entry: |G - G_ref| <= (1e-12 + q) C[j][j'], |b - b_ref| <= (1e-12 + q) sum_k |K_kj y_k| (Fourier: the weight sums of
# _phase_ref.fourier_gram_exact).  1e-12 is the stated tolerance of these forms (csrc/nufft.hip's header); at N = 4096 it also
# covers the direct sums' (N + 16) u = 4.6e-13.  q holds only the squares the kernel headers name, from the inputs in long double
# (_phase_ref.second_order): ((2 emax + |delta|) max|x|)^2 / 2 and (u max|w| max|x|)^2 / 2; q <= 1e-13 is asserted.  NOTHING grows with |w||x|.
# (id, Nf, Nv, grid, max|x|, a / D, planted max|eps| max|x|, signals)
PHASE_XMAX = 2.0e4
PHASE_LPV_CASES = [
    ("bench-24x3", 24, 3, "natural", PHASE_XMAX, 1.0, 0.0, 1),         # w = 2 pi (1 .. Nf) 25 / Nf: natural rounding residuals, |w x| to 3.1e6 rad
    ("bench-20x8", 20, 8, "natural", PHASE_XMAX, 1.0, 0.0, 1),
    ("bench-24x3-multi", 24, 3, "natural", PHASE_XMAX, 1.0, 0.0, 3),   # lpv_multi: the rhs calls reuse coordinates and binning
    ("beyond-24x3", 24, 3, "dyadic", None, 1.0, 0.0, 1),               # w = k 93 / 128: eps = 0 exactly, max|w x| = 2^30 rad
    ("resid-a=D", 24, 3, "natural", PHASE_XMAX, 1.0, 0.9e-7, 1),       # merged, s0 = 2: rhs on the grid
    ("resid-a=1.5D", 24, 3, "natural", PHASE_XMAX, 1.5, 0.9e-7, 1),    # merged, s0 = 3: rhs direct, delta != 0 allowed
    ("resid-a=0", 24, 3, "natural", PHASE_XMAX, 0.0, 0.9e-7, 1),       # merged, s0 = 0: zero frequency
    ("resid-split", 24, 3, "natural", PHASE_XMAX, 1.37, 0.9e-7, 1),    # 2a is no multiple of D: two slot families, ap in both modes
]
# predict's type-2 path (tests/test_gpu_predict.py): the (24, 3) shape from a = 2.5 D, so that the rotation e^{i a x} reaches 3.3e5 rad and
# the FMA error of a x, half an ulp of 2^18, is 2.9e-11 rad -- more than ten times the bound (from a = D it would be seven times; from
# a = 2 D the step of this grid happens to be a double, and its low word zero)
PHASE_PREDICT_CASES = [
    ("predict-24x3", 24, 3, "natural", PHASE_XMAX, 2.5, 0.0, 1),
    ("predict-24x3-residuals", 24, 3, "natural", PHASE_XMAX, 2.5, 0.9e-7, 1),
    ("predict-24x3-beyond", 24, 3, "dyadic", None, 1.0, 0.0, 1),
]
PHASE_LPV = {c[0]: c for c in PHASE_LPV_CASES + PHASE_PREDICT_CASES}
PHASE_N = 4096


def phase_lpv_inputs(case):
    """(Y, X, V, w): X unsorted, both signs, full-mantissa doubles; Y (N,) or (N, ns)."""
    cid, Nf, Nv, grid, xmax, a_over_D, resid, ns = case
    rng = np.random.default_rng(4000 + 10 * Nf + Nv + int(100 * a_over_D) + (7 if resid else 0))
    N = PHASE_N
    if grid == "dyadic":
        w = np.arange(1, Nf + 1) * (93.0 / 128.0)
        xmax = 2.0 ** 30 / w[-1]
    else:
        w = 2 * np.pi * (a_over_D + np.arange(Nf)) * 25.0 / Nf
    X = rng.uniform(-xmax, xmax, N)
    X[0], X[1] = xmax, -xmax                                       # the extremes are present
    V = rng.uniform(-1.0, 1.0, N)
    if resid:
        eps = rng.uniform(-1.0, 1.0, Nf)
        eps[0] = eps[-1] = 0.0
        w = w + eps * (resid / (np.abs(eps).max() * xmax))
    Y = rng.standard_normal((N, ns))
    return (Y[:, 0] if ns == 1 else Y), X, V, w


def phase_fourier_inputs(case):
    """STRUCT_FOURIER_CASES' shapes with full-mantissa stamps in [2^24, 2^24 + 300]: a window late in a long record."""
    cid, Nf, zero, weighted, N = case
    rng = np.random.default_rng(1700 + int(zero) + 2 * int(weighted))
    t = 2.0 ** 24 + np.sort(rng.random(N) * 300.0)
    f = (np.arange(Nf) if zero else np.arange(1, Nf + 1)) / 97.0
    y = np.sin(2 * np.pi * f[7] * (t - 2.0 ** 24)) + 0.2 * rng.standard_normal(N)
    return y, t, f, (rng.random(N) + 0.5 if weighted else None)


def phase_window_inputs():
    """(n, nwin, Nf, t, f, Y): three windows of 2048 samples late in a long record, t = 2^26 + k / 2 + jitter (full mantissa), 33 frequencies
    k / 68 (a = D: 72 merged slots, at least the 64 the batched transform asks for), two signals."""
    rng = np.random.default_rng(2048)
    n, nwin, Nf = 2048, 3, 33
    t = 2.0 ** 26 + 0.5 * np.arange(n * nwin) + 0.2 * rng.random(n * nwin)
    f = np.arange(1, Nf + 1) / 68.0
    Y = [np.sin(2 * np.pi * f[5 + 9 * q] * (t - 2.0 ** 26) + q) + 0.3 * rng.standard_normal(n * nwin) for q in range(2)]
    return n, nwin, Nf, t, f, Y
