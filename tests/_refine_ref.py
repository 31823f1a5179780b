"""Shared by tests/test_refine_ref_host.py and tests/test_gpu_refine.py: an exactly representable family of ill-conditioned systems, exact
residuals, and the bounds the refined solves of csrc/admm_refine.hip are held to.

The family.  B = (+)_k W_k diag(d_k) W_k' / m_k with W_k the Sylvester Hadamard matrix of order m_k (the powers of two of n's binary expansion,
largest first), d integers in [1, 2^20] with both ends present, and H = P B P' for one fixed permutation P applied to rows and columns alike, so that
every dense block is scattered over the whole matrix.  W_k / sqrt(m_k) is orthogonal: the eigenvalues of H are the d, cond(H) = 2^20 exactly.  x* holds
integers in [-8, 8] and b = H x*.  With m = max m_k, m H and m b are integers below 2^53 (asserted in int64), so H, b, x* and G = H - I -- the Gram a
handle is given with shift = 1/mu = 1; the same construction with d - 1 >= 0: singular, the shift holds it up -- are doubles without rounding.

Exact residuals.  b - H x for ANY double x: x is cut into 13-bit integer chunks x = sum_c X_c 2^(e_c); m H X_c is evaluated in int64 through two fast
Walsh-Hadamard transforms per block (|W' X_c| <= 2^25, times d <= 2^45, |W (...)| <= 2^57, times m / m_k: < 2^63), the chunks and b are combined in
Python integers at a common power of two, and the result is rounded ONCE (plus the rounded remainder: r = r_hi + r_lo to 2^-106).

Bounds.  u = 2^-53, gamma_k = (k + 16) u: a sum of k products in doubles in any order (the lanes' fma chains, the wave's shuffle tree) is within
gamma_k sum|terms|; the 16 covers the tree's six levels, the fma / subtract / add around the sum, the long-double reference's own rounding
(n 2^-64 <= 2 u per sum at n = 4096) and every second-order product of two of these terms.  A is the DEVICE's inverse (get_inverse(shift), row major as
the kernels read it), E = I - A H and E' = I - H A are formed in long double through the same transforms (error log2(m) 2^-64 per entry).  |H| is
|G| + I: the terms the residual kernels add (g_ii = h_ii - 1 >= 0, so the two agree).

 * Offset vector, one Dot2 step.  Device: xb0 = fl(A b); r^ = Dot2(b - G xb0 - shift xb0); t^ = fl(A r^); xb1 = fl(xb0 + t^).  Model: xb1 = xb0 + A r,
   r the exact residual of the device's xb0.  Dot2 (Ogita, Rump, Oishi 2005: "as if computed in twice the mantissa and rounded once"):
   |r^ - r| <= u |r| + gamma_n^2 (|b| + |H| |xb0|).  The product: |t^ - A r^| <= gamma_n |A| |r^|.  The sum: u |xb1|.  Together, componentwise,
       |xb1_dev - xb1_model| <= |A| (u |r| + gamma_n^2 (|b| + |H| |xb0|)) + gamma_n |A| |r| + u |xb1| ,
   and since xb1_model - x* = (I - A H)(xb0 - x*):   |xb1_dev - x*| <= |E| |xb0 - x*| + that bound.
   A residual formed in plain doubles has gamma_n (|b| + |H| |xb0|) in place of the first bracket: cond(H) times larger.

 * Ridge solve, two plain-double steps: x += fl(A fl(b - fl(G x) - ridge x)), twice.  Fixed-precision refinement does not improve the forward error;
   it makes the RESIDUAL small.  With r1 = b - H x1, r^1 = r1 + e_r, |e_r| <= gamma_(n+2) (|b| + |H| |x1|) (n products, the fma, the subtraction),
   d^ = A r^1 + e_A, |e_A| <= gamma_n |A| |r^1|, x2 = x1 + d^ + e_s, |e_s| <= u |x2|:
       b - H x2 = (I - H A) r1 - H A e_r - H e_A - H e_s ,
       |b - H x2| <= (gamma_(n+2) + u)(|b| + |H| |x2|) + |E'| |r1| + gamma_n |H| |A| |r1|
   to first order in e (H A = I - E', x1 = x2 up to d^); r1 is not observable on the device and is taken from the host model of the same recurrence.
   x0 = A b alone leaves |E'| |b| + gamma_n |H| |A| |b|: |H| |A| is far from |H A| = I on this family.

 * x-update correction.  Device: w = fl(A~ v), r^ = Dot2(v - H w), d = fl(A~ r^), xb_eff = fl(xb0 + d); the 8-byte storage has A~ = A.  Model:
   w = A v, d = A (v - H w), both in long double.  The device's w differs by dw, |dw| <= gamma_n |A| |v|, and the correction absorbs it:
   d_dev = d_model - A H dw.  Hence the offset-vector bound with b -> v, xb0 -> w, xb1 -> xb0 + d, plus |A| |H| gamma_n |A| |v|.  On this family
   |A| |H| has row sums of 1e5 and more, and that bound exceeds |d| itself: it cannot tell d from 0.  A H = I - E is known, so |A H dw| <=
   (I + |E|) gamma_n |A| |v| holds as well and is held too; with v a vector of small integers it is a tenth of |d|."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U = 2.0 ** -53
LOG2_COND = 20
CHUNK_BITS = 13
OFFSET_SIZES = (2048, 2100, 4096)             # np = 2048 (no pad), 2176 (76 pad rows), 4096 (symv_kernel<4>)
RIDGE_SIZES = (200, 513, 2100, 4096)          # + the full-matrix sizes below 2048, one of them odd with a block of order 1


def gamma(k):
    return (k + 16) * U


def padded_size(n):
    return -(-n // 128) * 128


def block_orders(n):
    return [1 << k for k in range(n.bit_length() - 1, -1, -1) if n >> k & 1]


def hadamard(m):
    """Sylvester's W_m (dense, int64): W_2m = [[W, W], [W, -W]]."""
    W = np.ones((1, 1), dtype=np.int64)
    while W.shape[0] < m:
        W = np.block([[W, W], [W, -W]])
    return W


def fwht(a):
    """W_m a along axis 0 (m a power of two) in a's own arithmetic: int64 exactly, long double with log2(m) roundings per entry."""
    m = a.shape[0]
    a = np.array(a).reshape(m, -1)
    h = 1
    while h < m:
        v = a.reshape(m // (2 * h), 2, h, -1)
        t = v[:, 0] - v[:, 1]
        v[:, 0] += v[:, 1]
        v[:, 1] = t
        h *= 2
    return a


def spectrum(n, rng):
    """Integers in [1, 2^20], log-uniform, both ends in the first (largest) block."""
    d = np.clip(np.floor(2.0 ** (LOG2_COND * rng.random(n))).astype(np.int64), 1, 1 << LOG2_COND)
    d[0], d[1] = 1, 1 << LOG2_COND
    return d


class Family:
    """H = P B P' of order n with nrhs right-hand sides; see the module docstring."""

    def __init__(self, n, nrhs=1):
        self.n, self.nrhs = n, nrhs
        self.orders = block_orders(n)
        self.m = self.orders[0]
        rng = np.random.default_rng(7000 + n)
        self.d = spectrum(n, rng)
        self.perm = rng.permutation(n)
        self.offsets = np.concatenate([[0], np.cumsum(self.orders)]).astype(np.int64)
        Hint = np.zeros((n, n), dtype=np.int64)                      # m H
        for o, mk in zip(self.offsets, self.orders):
            Hint[o:o + mk, o:o + mk] = fwht(self.d[o:o + mk, None] * hadamard(mk)) * (self.m // mk)      # W (D W'), W' = W
        inv = np.empty(n, dtype=np.int64)
        inv[self.perm] = np.arange(n)
        Hint = Hint[np.ix_(inv, inv)]                                # H[perm[k], perm[l]] = B[k, l]
        assert np.abs(Hint).max() < 2 ** 53 and np.array_equal(Hint, Hint.T)
        self.H = Hint.astype(np.float64) / self.m
        self.G = self.H - np.eye(n)
        assert np.array_equal(self.G + np.eye(n), self.H)
        self.xstar = np.random.default_rng(7100 + n).integers(-8, 9, (n, nrhs)).astype(np.float64)
        bint = self.apply_int(self.xstar.astype(np.int64))          # m b
        assert np.abs(bint).max() < 2 ** 53
        self.b = bint.astype(np.float64) / self.m
        self.absH = np.abs(self.G) + np.eye(n)

    def _apply(self, X, integer):
        Y = X[self.perm]
        Z = np.empty_like(Y)
        for o, mk in zip(self.offsets, self.orders):
            t = fwht(Y[o:o + mk]) * self.d[o:o + mk, None].astype(Y.dtype)
            t = fwht(t)
            Z[o:o + mk] = t * (self.m // mk) if integer else t / Y.dtype.type(mk)
        out = np.empty_like(Z)
        out[self.perm] = Z
        return out

    def apply_int(self, X):
        """m H X for an int64 array X [n, q], exactly (|X| <= 2^13 keeps every intermediate below 2^63)."""
        return self._apply(np.ascontiguousarray(X, dtype=np.int64).reshape(self.n, -1), True)

    def apply_ld(self, X, cols=512):
        """H X in long double through the transforms (2 log2(m) + 2 roundings per entry instead of n)."""
        X = np.asarray(X, dtype=np.longdouble).reshape(self.n, -1)
        parts = [np.ascontiguousarray(X[:, c:c + cols]) for c in range(0, X.shape[1], cols)]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:          # (numpy's loops release the interpreter lock)
            return np.concatenate(list(pool.map(lambda part: self._apply(part, False), parts)), axis=1)


@functools.lru_cache(maxsize=None)
def family(n, nrhs=1):
    return Family(n, nrhs)


# ---- exact residual ---------------------------------------------------------------------------------------------------------------------
def _exact_ints(a):
    """Doubles as (integer mantissa, exponent): a = M 2^e exactly."""
    mant, ex = np.frexp(a)
    return (mant * 2.0 ** 53).astype(np.int64), ex.astype(np.int64) - 53


def _round_pair(R, E):
    """The integer R times 2^E as hi + lo, hi the correctly rounded double, lo the rounded remainder."""
    def to_float(v):
        return v / (1 << -E) if E < 0 else float(v << E)
    hi = to_float(R)
    p, q = hi.as_integer_ratio()
    hi_int = (p << -E) // q if E < 0 else p // (q << E)
    return hi, to_float(R - hi_int)


def exact_residual(F, b, x):
    """b - H x for doubles b, x [n] or [n, q], exactly: -> (r_hi, r_lo), r_hi the residual rounded once."""
    shape = np.shape(x)
    b = np.asarray(b, dtype=np.float64).reshape(F.n, -1)
    rem = np.array(x, dtype=np.float64).reshape(F.n, -1)
    assert np.all(np.isfinite(rem)) and np.all(np.isfinite(b))
    xmax = float(np.abs(rem).max())
    e = int(np.ceil(np.log2(xmax))) + 1 if xmax > 0 else 0
    acc = np.zeros(rem.shape, dtype=object)                          # m H x / 2^e, Horner over the chunks
    while np.any(rem):
        e -= CHUNK_BITS
        q = 2.0 ** e
        xc = np.rint(rem / q)
        assert np.abs(xc).max() <= 2 ** CHUNK_BITS
        rem = rem - xc * q                                           # exact: the bits of rem below q
        acc = acc * (1 << CHUNK_BITS) + F.apply_int(xc.astype(np.int64)).astype(object)
    e -= F.m.bit_length() - 1                                        # H x = acc 2^e
    Mb, eb = _exact_ints(b)
    E = int(min(e, eb[Mb != 0].min() if np.any(Mb) else e))
    hi, lo = np.empty(rem.shape), np.empty(rem.shape)
    Mb, eb, accf = Mb.ravel().tolist(), eb.ravel().tolist(), acc.ravel().tolist()
    hf, lf = hi.reshape(-1), lo.reshape(-1)
    for i, (mb, ebi, a) in enumerate(zip(Mb, eb, accf)):
        R = (mb << (ebi - E) if mb else 0) - (int(a) << (e - E))
        hf[i], lf[i] = _round_pair(R, E)
    return hi.reshape(shape), lo.reshape(shape)


# ---- what the bounds need of the device's inverse -----------------------------------------------------------------------------------
class Inverse:
    """A = the inverse in use, row major (A[i, j] multiplies b[j] in row i): |A|, E = I - A H, E' = I - H A and their absolute values."""

    def __init__(self, F, A):
        self.F = F
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.absA = np.abs(self.A)

    def _defect(self, X):
        P = self.F.apply_ld(X)
        P[np.diag_indices(self.F.n)] -= 1
        return np.abs(P).astype(np.float64)

    @functools.cached_property
    def absE(self):
        return np.ascontiguousarray(self._defect(self.A.T).T)                        # A H = (H A')'

    @functools.cached_property
    def absEp(self):
        return self._defect(self.A)

    @functools.cached_property
    def normE(self):
        return float(self.absE.sum(axis=1).max())

    @functools.cached_property
    def Ald(self):
        return self.A.astype(np.longdouble)

    def apply_ld(self, v):
        """A v in long double, rounded to double."""
        return (self.Ald @ np.asarray(v).astype(np.longdouble)).astype(np.float64)

    def apply2_ld(self, hi, lo):
        """A (hi + lo) in long double."""
        return self.Ald @ (np.asarray(hi).astype(np.longdouble) + np.asarray(lo).astype(np.longdouble))


def offset_model(F, inv, b, xb0):
    """One exact refinement step of xb0: -> dict(xb1, bound), bound componentwise on |xb1_dev - xb1|."""
    n = F.n
    r_hi, r_lo = exact_residual(F, b, xb0)
    xb1 = np.asarray(xb0).astype(np.longdouble) + inv.apply2_ld(r_hi, r_lo)          # (kept in long double: the model is not rounded to the grid it judges)
    absr = np.abs(r_hi)
    bound = inv.absA @ (U * absr + gamma(n) ** 2 * (np.abs(b) + F.absH @ np.abs(xb0))) + gamma(n) * (inv.absA @ absr) + U * np.abs(xb1).astype(np.float64)
    return dict(xb1=xb1, bound=bound)


def offset_forward_bound(F, inv, xb0, xstar, bound):
    return inv.absE @ np.abs(xb0 - xstar) + bound


def product_bound(F, inv, b):
    """|fl(A b) - A b| componentwise."""
    return gamma(F.n) * (inv.absA @ np.abs(b))


def ridge_recurrence(F, inv, b, steps, residual="double"):
    """x0 = A b and `steps` refinement steps in host doubles: -> [x0, x1, ...].  residual = "double" (the device's ridge solve), "longdouble"
    (a 64-bit-mantissa residual, rounded to double) or "exact" (rounded once: what Dot2 promises)."""
    xs = [inv.A @ b]
    for _ in range(steps):
        x = xs[-1]
        if residual == "double":
            r = b - (F.G @ x + x)
        elif residual == "longdouble":
            xl = x.astype(np.longdouble)
            r = (b.astype(np.longdouble) - (F.G.astype(np.longdouble) @ xl + xl)).astype(np.float64)
        else:
            r = exact_residual(F, b, x)[0]
        xs.append(x + inv.A @ r)
    return xs


def ridge_residual_bound(F, inv, b, x2, r1):
    """Componentwise bound on |b - H x2| after two plain-double steps; r1 = the exact residual of the model's x1."""
    n = F.n
    absr1 = np.abs(r1)
    return ((gamma(n + 2) + U) * (np.abs(b) + F.absH @ np.abs(x2)) + inv.absEp @ absr1 + gamma(n) * (F.absH @ (inv.absA @ absr1)))


def correction_model(F, inv, v, xb0):
    """-> dict(w, d, bound, bound_tight): d = A (v - H w), w = A v in long double; bounds componentwise on |(xb_eff - xb0)_dev - d|.
    `bound` carries the absorbed rounding of w as |A| |H| gamma_n |A| |v|; `bound_tight` as (I + |E|) gamma_n |A| |v| (A H = I - E, no
    triangle inequality through |A| |H|: five orders of magnitude smaller on this family, and the one that tells d from 0)."""
    n = F.n
    w = inv.apply_ld(v)
    r_hi, r_lo = exact_residual(F, v, w)
    d = inv.apply2_ld(r_hi, r_lo)                                                    # (long double)
    absr = np.abs(r_hi)
    base = (inv.absA @ (U * absr + gamma(n) ** 2 * (np.abs(v) + F.absH @ np.abs(w))) + gamma(n) * (inv.absA @ absr) + U * np.abs(xb0 + d.astype(np.float64)))
    dw = gamma(n) * (inv.absA @ np.abs(v))
    return dict(w=w, d=d, bound=base + inv.absA @ (F.absH @ dw), bound_tight=base + dw + inv.absE @ dw)


def worst_ratio(err, bound):
    """max |err| / bound; where the bound is zero the error must be."""
    err, bound = np.abs(np.asarray(err)).astype(np.float64), np.asarray(bound)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


# ---- a spectrum no refinement in doubles survives (the refusal case) -----------------------------------------------------------------
def hopeless(n=200, log2cond=50):
    """The same construction with d = 2^k, k spread over [0, log2cond] (built in doubles: not exact, and it need not be) -> (H, b)."""
    F = family(n)
    k = np.round(np.linspace(0, log2cond, n)).astype(np.int64)
    np.random.default_rng(9).shuffle(k)
    B = np.zeros((n, n))
    for o, mk in zip(F.offsets, F.orders):
        W = hadamard(mk).astype(np.float64)
        B[o:o + mk, o:o + mk] = (W * 2.0 ** k[o:o + mk]) @ W.T / mk
    inv = np.empty(n, dtype=np.int64)
    inv[F.perm] = np.arange(n)
    H = B[np.ix_(inv, inv)]
    H = 0.5 * (H + H.T)
    return H, H @ F.xstar[:, 0]


def eigenvector_rhs(n=200, log2cond=36):
    """A right-hand side the residual test must refuse although every pivot is safe -> (H, b).  The same construction with d = 2^k, k spread over
    [0, log2cond] (m H < 2^53: exact), and x* the +-1 Hadamard column of the first block that belongs to d = 1, so that b = H x* = x* exactly.  The
    residual of any x near x* formed in doubles carries the rounding of H x, about sqrt(n) u |H|_2 |x| = 1e-5 against |b| = |x|: four decades above the
    1e-9 the solve accepts, whatever the refinement does.  gamma_n |H|_2 = 1.6e-3 is far below lambda_min = 1: an elimination without pivoting keeps
    its pivots positive (Higham, Accuracy and Stability, Thm 10.7)."""
    F = family(n)
    m0 = F.orders[0]
    k = np.round(np.linspace(0, log2cond, n)).astype(np.int64)
    np.random.default_rng(9).shuffle(k)
    j, i = int(np.argmin(k[:m0])), int(np.argmin(k))
    k[j], k[i] = k[i], k[j]                                         # a unit eigenvalue inside the first block
    d = np.int64(1) << k
    Hint = np.zeros((n, n), dtype=np.int64)
    for o, mk in zip(F.offsets, F.orders):
        Hint[o:o + mk, o:o + mk] = fwht(d[o:o + mk, None] * hadamard(mk)) * (F.m // mk)
    assert np.abs(Hint).max() < 2 ** 53
    inv = np.empty(n, dtype=np.int64)
    inv[F.perm] = np.arange(n)
    H = Hint[np.ix_(inv, inv)].astype(np.float64) / F.m
    xs = np.zeros(n)
    xs[F.perm[:m0]] = hadamard(m0)[:, j]
    b = H @ xs
    assert np.array_equal(b, xs)
    return H, b
