"""Host model (numpy, f64) of the second half of the ADMM step -- z = prox(x + u), u += x - z, rhs = (z - u)/mu, ||x - z||, stop if
< tol -- with the operation order of oracle/lpvs_oracle.c (prox operators) and src/lasso.jl:152-164, and the input generators the host and
the GPU tests share (tests/test_prox_ref_host.py, tests/test_gpu_prox_update.py).  Nothing here touches the device.

Every floating-point operation below is one IEEE double operation, the same one the kernels perform (the library is built with
-ffp-contract=off); sums are sequential where the kernels' are.  Signed zeros are not part of the contract: compare with `==`.
"""
import numpy as np

L1, L0, BALL, GROUP = 1, 2, 3, 4
U = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- the model
def group_s2(v, gl):
    """Per whole group: the sum of the ROUNDED squares, added sequentially from zero (norm() on a short slice)."""
    ng = v.size // gl
    sq = (v[:ng * gl] * v[:ng * gl]).reshape(ng, gl)
    s2 = np.zeros(ng)
    with np.errstate(over="ignore"):
        for q in range(gl):
            s2 = s2 + sq[:, q]
    return s2


def ball_keep(v, r):
    """Mask of the r largest |v|, ties to the lowest index (a stable sort of -|v|)."""
    n = v.size
    keep = np.zeros(n, dtype=bool)
    if r >= n:
        keep[:] = True
    elif r > 0:
        keep[np.argsort(-np.abs(v), kind="stable")[:r]] = True
    return keep


def prox(kind, v, param, mu, gl=0, z_prev=None):
    v = np.asarray(v, dtype=np.float64)
    if kind == L1:
        g = mu * param
        return v + np.where(v <= -g, g, np.where(v >= g, -g, -v))
    if kind == L0:
        return np.where(np.abs(v) > np.sqrt(2.0 * mu * param), v, 0.0)
    if kind == BALL:
        return np.where(ball_keep(v, int(param)), v, 0.0)
    assert kind == GROUP and gl >= 1
    ng = v.size // gl
    z = np.zeros(v.size) if z_prev is None else np.array(z_prev, dtype=np.float64)   # entries beyond the last whole group keep z
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        scale = 1.0 - (param * mu) / np.sqrt(group_s2(v, gl))                            # s2 == 0 -> -inf -> 0
        scale = np.where(scale > 0, scale, 0.0)                                          # !(scale > 0) -> 0
        z[:ng * gl] = np.repeat(scale, gl) * v[:ng * gl]
    return z


def sum_is_exact(d):
    """True when sum d^2 is exact in ANY order: every d is an integer multiple k of one power of two and n max(k)^2 < 2^53, so every
    square and every partial sum is an integer below 2^53 in units of that power's square."""
    d = np.abs(np.asarray(d, dtype=np.float64))
    d = d[d != 0]
    if d.size == 0:
        return True
    m, e = np.frexp(d)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = e - 53 + np.round(np.log2((mi & -mi).astype(np.float64))).astype(np.int64)   # exponent of the lowest set bit
    k = float(d.max()) / 2.0 ** int(low.min())
    return k * k * (d.size + 1) < 2.0 ** 53


def step(z0, u0, mu, kind, param, gl=0):
    """One iteration through M = mu I from the state (z0, u0): every intermediate."""
    with np.errstate(over="ignore", invalid="ignore"):
        rhs0 = (z0 - u0) / mu
        x = mu * rhs0                      # one non-zero product per row, added to zeros
        v = x + u0
        z = prox(kind, v, param, mu, gl, z_prev=z0)
        d = x - z
        u = u0 + d
        rhs = (z - u) / mu
        d2 = d * d
    exact = sum_is_exact(d)
    nxz = float(np.sqrt(np.sum(d2) if exact else np.sum(d2.astype(np.longdouble))))
    return dict(x=x, v=v, z=z, d=d, u=u, rhs=rhs, nxz=nxz, nxz_exact=exact)


def iterate(z0, u0, mu, kind, param, gl=0, tol=0.0, iters=1):
    """`iters` iterations with the reference's stopping test (src/lasso.jl:164: strict <, in the iteration it belongs to): the final
    x, z, u, the per-iteration records, the count of iterations done and the converged flag."""
    z, u = np.array(z0, dtype=np.float64), np.array(u0, dtype=np.float64)
    x = np.zeros_like(z)
    hist, conv = [], False
    for _ in range(iters):
        s = step(z, u, mu, kind, param, gl)
        hist.append(s)
        x, z, u = s["x"], s["z"], s["u"]
        if s["nxz"] < tol:
            conv = True
            break
    return dict(x=x, z=z, u=u, hist=hist, iters=len(hist), converged=conv, nxz=hist[-1]["nxz"] if hist else 0.0,
                nxz_exact=hist[-1]["nxz_exact"] if hist else True)


def nxz_bound(n):
    """Relative bound on a computed ||d|| whose squares and sums round: n - 1 additions and one product per term in any order, and the
    square root: (n + 2) 2^-53 to first order, halved by the root, not halved here."""
    return (n + 2) * U


# ------------------------------------------------------------------------------------------------------- input generators
def dyadic(n, rng, bits=40, lo=0.0, hi=8.0):
    """Integers x 2^-bits with lo <= |.| < hi, random signs."""
    k = rng.integers(int(lo * 2 ** bits), int(hi * 2 ** bits), n).astype(np.float64)
    return np.where(rng.random(n) < 0.5, -1.0, 1.0) * k * 2.0 ** -bits


def edge_positions(n):
    """Index 0, n - 1 and both sides of every multiple of 128 (n - 1 sits next to the pad rows when n % 128 != 0)."""
    pos = [0]
    for m in range(128, n, 128):
        pos += [m - 1, m]
    pos.append(n - 1)
    return sorted(set(pos))


def cut_values(c, f32=False):
    """The seven values around a cut c > 0: the cut, its two neighbours (in the I/O type of the handle), both signs, and zero."""
    t = np.float32 if f32 else np.float64
    up, dn = float(np.nextafter(t(c), t(np.inf))), float(np.nextafter(t(c), t(0.0)))
    return [c, -c, up, -up, dn, -dn, 0.0]


L1_CUT = dict(kind=L1, mu=2.0 ** -4, param=4.0)        # g = mu lambda = 0.25
L0_CUT = dict(kind=L0, mu=2.0 ** -3, param=1.0)        # sqrt(2 mu lambda) = 0.5 exactly


def cuts(n, rng, c, shift=0, f32=False):
    """Dense coarse dyadic values with the seven cut values cycled over the edge positions (7 is odd and the positions alternate sides of
    a boundary, so both sides of a boundary see every value over the boundaries); returns (v, positions that hold a cut value)."""
    v = dyadic(n, rng, bits=12, hi=2.0)
    pos = edge_positions(n)
    pos = sorted(set(pos) | set(range(n // 2 - 5, n // 2 + 5))) if len(pos) < 14 else pos   # (few boundaries: interior positions too, so that
    vals = cut_values(c, f32)                                                               #  every value occurs at least twice)
    for j, i in enumerate(pos):
        v[i] = vals[(j + shift) % 7]
    return v, np.array(pos)


GROUP_MU, GROUP_LAM = 2.0 ** -4, 5.0                   # lambda mu = 5 * 2^-4: the norm of (3, 4, 0, ...) * 2^-4, exactly


def group_input(n, gl, rng, with_next=True, bits=40):
    """Dense groups (|v| in [1, 8), 2^-bits grid) with the special groups cycled over group 0, the last whole group and the groups on both
    sides of every multiple of 128 (of few, long groups only the odd ones: the others stay dense): norm exactly lambda mu (z = 0), the next s2 above it (gl >= 3; the closest above for gl < 3), an
    all-zero group, a one-hot group.  Returns (v, number of special groups)."""
    ng = n // gl
    v = dyadic(n, rng, bits=bits, lo=1.0, hi=8.0)
    t = GROUP_LAM * GROUP_MU                            # 0.3125
    groups = sorted({0, ng - 1} | {min(i // gl, ng - 1) for i in edge_positions(n)})
    if 2 * len(groups) > ng:                             # few, long groups: at most every second one is special, the others stay dense
        groups = [g for g in groups if g % 2 == 1 or ng >= 2 * len(groups)]
    kinds = ["exact", "next", "zero", "onehot"] if with_next else ["exact", "zero", "onehot"]
    up = (lambda a: float(np.nextafter(np.float32(a), np.float32(1.0)))) if bits <= 20 else (lambda a: float(np.nextafter(a, 1.0)))
    for j, g in enumerate(groups):
        blk = np.zeros(gl)
        k = kinds[j % len(kinds)]
        if k in ("exact", "next"):
            if gl == 1:
                blk[0] = -t if k == "exact" else up(t)
            else:
                blk[0], blk[-1] = 3 * t / 5, -4 * t / 5                 # s2 = 25 * 2^-8, ulp 2^-56
                if k == "next":
                    if gl >= 3:
                        blk[1] = 2.0 ** -28                              # + 2^-56: the next representable s2
                    else:
                        blk[-1] = -up(4 * t / 5)
        elif k == "onehot":
            blk[(j * 7) % gl] = -2.5
        v[g * gl:(g + 1) * gl] = blk
    return v, len(groups)


def ball_inputs(n, rng, big=False):
    """[(label, v, [r ...], number of tie / cut elements)]: one case per selection level of admm_prox_kernel.  `big`: only
    the cases that matter at n > 32768 (the entry straight into the 64-bit select)."""
    out = []
    perm = rng.permutation(n)
    distinct = (perm + 1.0) * 2.0 ** -12 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    out.append(("distinct", distinct, [1, 2, 32, n // 2, n - 1, n, n + 5], 0))
    K = 5                                               # distinct values above every special set

    def base():
        v = dyadic(n, rng, bits=30, hi=0.25)
        top = rng.choice(n, K, replace=False)
        v[top] = (4.0 + np.arange(K)) * np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
        return v, set(int(i) for i in top)

    def free(v, taken, want):
        """`want` ascending indices not in `taken`, nudged upwards."""
        got = []
        for i in want:
            while i in taken or i in got:
                i += 1
            got.append(i)
        return got

    # exact ties of |v| with mixed signs, winners and losers in different 1024-thread chunks / 8192-element passes
    v, taken = base()
    want = [5, 1030, 1100, n // 2, n - 3] + ([8200, 8300] if n > 8300 else [700]) + ([32770] if n > 32770 else [])
    idx = sorted(free(v, taken, want))
    v[idx] = 3.0 * np.where(np.arange(len(idx)) % 2 == 0, 1.0, -1.0)
    T = len(idx)
    out.append(("ties", v, [K + 1, K + T // 2, K + T - 1], T))
    # a sparse v: the cut falls among the exact zeros, the survivors are the non-zeros
    v = np.zeros(n)
    nz = rng.choice(n, 40, replace=False)
    v[nz] = dyadic(40, rng, bits=20, lo=0.5, hi=4.0)
    out.append(("sparse", v, [41], n - 40))
    if big:
        return out
    # 2 - 2^-30, 2, 2 + 2^-30: one float key (2.0f); the larger the value the higher its index
    v, taken = base()
    idx = free(v, taken, [n // 3, n // 3 + 1030, n - 2])
    v[idx] = [-(2.0 - 2.0 ** -30), 2.0, -(2.0 + 2.0 ** -30)]
    out.append(("one-float-key-3", v, [K + 1, K + 2], 3))
    for m in (1023, 1024):
        # m elements inside one 11-bit bin (exponent + 3 mantissa bits): the fast path's last size and its first fall-back
        v, taken = base()
        idx = np.array([i for i in rng.permutation(n) if i not in taken][:m])
        v[idx] = (1.0 + np.arange(m) * 2.0 ** -20) * np.where(np.arange(m) % 3 == 0, -1.0, 1.0)
        out.append((f"bin11-{m}", v, [K + m // 2, K + 1, K + m - 1], m))
        # m elements with one float key and distinct doubles: the byte-wise fall-back's last size and the first 64-bit select
        v2 = v.copy()
        v2[idx] = (1.0 + np.arange(m) * 2.0 ** -45) * np.where(np.arange(m) % 3 == 0, -1.0, 1.0)
        out.append((f"float-key-{m}", v2, [K + m // 2, K + 1], m))
        # ... and with exact ties at the threshold: Q levels of (up to) four equal |v| a quarter of the index range apart, the cut inside a
        # quadruple.  r = K + 402 keeps two of the four elements of level Q - 101; beyond n = 8192 its two last members are moved behind
        # index 8192, so that the kept and the dropped ones lie in different 8192-element passes (the carried count of equal keys)
        v3 = v.copy()
        sidx = np.sort(idx)
        Q = (m + 3) // 4
        level = np.arange(m) % Q
        v3[sidx] = (1.0 + level * 2.0 ** -45) * np.where(np.arange(m) % 3 == 0, -1.0, 1.0)
        if n > 8300:
            members = sidx[level == Q - 101]
            assert members.size == 4 and members[1] < 8192
            for old, new in zip(members[2:], free(v3, taken | set(int(i) for i in sidx), [8200, 8300])):
                v3[new], v3[old] = v3[old], 2.0 ** -10
        out.append((f"float-key-ties-{m}", v3, [K + 402, K + 4 * 37 + 1], m))
    return out


def wide_values(n, rng):
    """|v| from 2^-1060 to 2^990, random signs, a few exact zeros."""
    e = rng.integers(-1060, 991, n)
    v = np.ldexp(1.0 + rng.integers(0, 2 ** 20, n) * 2.0 ** -20, e) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    v[rng.choice(n, 5, replace=False)] = 0.0
    return v


def wide_ball(n, rng):
    """Values above FLT_MAX (float key +inf) and below 2^-149 (float key 0), the cut between them: [(label, v, [r ...], count)]."""
    v = dyadic(n, rng, bits=20, lo=0.5, hi=4.0)
    hi = rng.choice(n, 6, replace=False)
    v[hi] = np.ldexp([1.0, -1.5, 1.25, -1.0, 1.75, 1.0], [200, 200, 300, 129, 128, 500])
    out = [("above-FLT_MAX", v, [1, 3, 5], 6)]
    v = np.zeros(n)
    lo = rng.choice(n, 8, replace=False)
    v[lo] = np.ldexp([1.0, -1.5, 1.25, -1.0, 1.75, 1.0, -1.0, 1.5], [-200, -200, -300, -150, -151, -500, -1060, -1074])
    out.append(("below-2^-149", v, [2, 4, 7], 8))
    return out


def wide_group(n, gl, rng):
    """A group whose s2 overflows (scale = 1, z = v) and one whose s2 underflows to 0 (z = 0) among dense groups."""
    v = dyadic(n, rng, bits=40, lo=1.0, hi=8.0)
    ng = n // gl
    g1, g2 = 1 % ng, ng - 1
    v[g1 * gl:(g1 + 1) * gl] = np.ldexp(dyadic(gl, rng, bits=10, lo=1.0, hi=2.0), 600)
    v[g2 * gl:(g2 + 1) * gl] = np.ldexp(dyadic(gl, rng, bits=10, lo=1.0, hi=2.0), -600)
    return v
