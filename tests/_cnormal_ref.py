"""Plain numpy restatement of the reference's ComplexNormal (src/utilities.jl:80-174), detrend (src/utilities.jl:1-17) and the numbers
of the SpectralExt plot recipe (src/plotting.jl:54-106), written from the reference line by line, plus a pure-Python Philox4x32-10
and Box-Muller written from the published algorithm (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Box & Muller
1958).  The reference cannot run where the tests run (no Julia): this file is the reference of tests/test_cnormal_host.py and
tests/test_gpu_cnormal.py.  It does not import the package under test.
"""
import numpy as np


# ---- detrend ---------------------------------------------------------------------------------------------------------------------------
def detrend(x, order=0, t=None):
    y = np.array(x, dtype=np.float64)                      # src/utilities.jl:15  y = copy(x)
    t = np.arange(1, len(y) + 1, dtype=np.float64) if t is None else np.asarray(t, dtype=np.float64)   # :1  t = 1:length(x)
    y = y - np.mean(x)                                     # :2  x[:] .-= mean(x)
    if order == 1:                                         # :3
        k = np.dot(y, t) / np.dot(y, y)                    # :4  k = x\t (vector \ vector: the least-squares scalar (x.t)/(x.x))
        y = y - k * t                                      # :5  x[:] .-= k*t
    return y


# ---- ComplexNormal ---------------------------------------------------------------------------------------------------------------------
def symmetric(V):
    """Symmetric(V): the upper triangle decides (uplo = :U)."""
    V = np.asarray(V)
    return np.triu(V) + np.triu(V, 1).T


def hermitian(A):
    A = np.asarray(A)
    return np.triu(A, 1) + np.triu(A, 1).conj().T + np.diag(np.diag(A).real)


def chol_upper(A):
    """cholesky(A).U"""
    return np.linalg.cholesky(hermitian(A)).conj().T


def cn_V2GC(V):
    V = symmetric(np.asarray(V, dtype=np.float64))         # src/utilities.jl:124
    n = V.shape[0] // 2                                    # :114
    Vxx = V[:n, :n]                                        # :115
    Vyy = V[n:, n:]                                        # :116
    Vxy = V[:n, n:]                                        # :117
    Vyx = V[n:, :n]                                        # :118
    G = (Vxx + Vyy) + 1j * (Vyx - Vxy)                     # :119  (the reference keeps cholesky(G); Matrix(G) is G up to rounding)
    C = symmetric((Vxx - Vyy) + 1j * (Vyx + Vxy))          # :120
    return G, C


def cn_fVxx(G, C): return (G + C).real / 2                 # :131
def cn_fVyy(G, C): return (G - C).real / 2                 # :132
def cn_fVxy(G, C): return (-G + C).imag / 2                # :133
def cn_fVyx(G, C): return (G + C).imag / 2                 # :134
def cn_fV(G, C): return np.block([[cn_fVxx(G, C), cn_fVxy(G, C)], [cn_fVyx(G, C), cn_fVyy(G, C)]])   # :137
def cn_V(G, C): return chol_upper(cn_fV(G, C))             # :138


def from_samples(X, Y):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    assert X.shape == Y.shape                              # :90
    mc = X.mean(axis=0) + 1j * Y.mean(axis=0)              # :91
    V = symmetric(np.cov(np.concatenate([X, Y], axis=1), rowvar=False, ddof=1))   # :92
    G, C = cn_V2GC(V)                                      # :93
    return mc, G, C, V


def from_mean_cov(m, V):
    m = np.asarray(m)
    if not np.iscomplexobj(m):                             # :101-106
        n = len(m) // 2
        m = m[:n] + 1j * m[n:]
    G, C = cn_V2GC(V)                                      # :104 / :109
    return m, G, C


def pdf(m, G, C, z):
    z = np.asarray(z, dtype=np.complex128)
    k = len(m)                                             # :152
    R = np.conj(C).conj().T @ np.linalg.inv(G)             # :153
    P = G - R @ C                                          # :154
    cm = np.conj(m)                                        # :155
    cz = np.conj(z)                                        # :156
    zmm = z - m                                            # :157
    czmm = cz - cm                                         # :158
    ld = np.concatenate([np.conj(czmm), np.conj(zmm)])     # :159  [czmm' zmm']
    rd = np.concatenate([zmm, czmm])                       # :160
    S = np.block([[G, C], [np.conj(C), G]])                # :161
    detG = float(np.prod(np.diag(chol_upper(G)).real) ** 2)   # det(::Cholesky)
    return 1 / (np.pi ** k * np.sqrt(detG * np.linalg.det(P) + 0j)) * np.exp(-0.5 * (ld @ np.linalg.solve(S, rd)))   # :162


def affine_transform(m, G, C, A, b):
    A = np.asarray(A)
    return A @ m + b, hermitian(A @ G @ np.conj(A.T)), symmetric(A @ C @ A.T)   # :165


def rand_given(m, U, R, dtype=np.float64):
    """rand(cn, s) with randn(s, 2n) = R and L = U given (src/utilities.jl:168-174)."""
    m = np.asarray(m)
    mm = np.concatenate([m.real, m.imag]).astype(dtype)    # :170
    n = len(m)                                             # :171
    z = mm[None, :] + np.asarray(R, dtype=dtype) @ np.asarray(U, dtype=dtype)   # :172
    return z[:, :n], z[:, n:]                              # :173 (real and imaginary parts of the complex result)


# ---- the recipe --------------------------------------------------------------------------------------------------------------------------
def linrange(a, b, n):
    t = np.arange(n) / (n - 1)
    return (1 - t) * a + t * b                             # LinRange: lerpi


def basis_activation(V, Nv, normalize, coulomb):
    """src/utilities.jl:23-36 with the kernels of src/lsfft.jl:195-207; returns K(v) for a vector v (rows)."""
    V = np.asarray(V, dtype=np.float64)
    if coulomb:
        vc = np.linspace(0, np.max(np.abs(V)), Nv + 2)[1:-1]   # :25-26
        vc = np.concatenate([-vc[::-1], vc])                   # :27
        nb = 2 * Nv                                            # :28
        gamma = nb / abs(vc[0] - vc[-1])                       # :29
    else:
        vc = np.linspace(V.min(), V.max(), Nv)                 # :32
        gamma = Nv / abs(vc[0] - vc[-1])                       # :33

    def K(v):
        v = np.atleast_1d(np.asarray(v, dtype=np.float64))
        r = np.exp(-gamma * (v[:, None] - vc[None, :]) ** 2)   # src/lsfft.jl:195  _K
        if coulomb:
            r = np.where(np.sign(v)[:, None] == np.sign(vc)[None, :], r, 0.0)   # :202  _Kcoulomb: sign.(V) .== sign.(vc)
        if normalize:
            r = r / r.sum(axis=1, keepdims=True)               # :199 / :206
        return r
    return K


def schedfunc(x, Sigma, V, w, Nv, normalize, coulomb, R=None, U=None, nMC=5000, phase=False, normalization="none", normdim="freq", K=None):
    """F, P, FBl, FBu, FBm, PBl, PBu, PBm, vg and the amplitudes / phases of all draws (FB, PB) given the normals R and the factor U
    (src/plotting.jl:54-106).  K: the grid table (G x nb) when the caller evaluates the basis elsewhere."""
    w = np.asarray(w, dtype=np.float64)
    Nf = len(w)                                            # :56
    xm = np.reshape(np.asarray(x), (Nf, -1), order="F")    # :57
    V = np.asarray(V, dtype=np.float64)
    G = 101 if Nf == 100 else 100
    vg = linrange(V.min(), V.max(), G)                     # :62
    Kg = basis_activation(V, Nv, normalize, coulomb)(vg) if K is None else np.asarray(K)   # :60, :75
    d = np.conj(xm) @ Kg.T                                 # :76  dot(x[j,:], phi) conjugates x
    F = np.abs(d)                                          # :76
    P = np.angle(d)                                        # :77
    out = dict(vg=vg, F=F, P=P, K=Kg)
    if R is not None:                                      # :68-71
        zr, zi = rand_given(np.asarray(x).ravel(), U, R)   # :70
        z = zr + 1j * zi
        n = z.shape[1]
        nb = n // Nf
        FB = np.zeros((Nf, G, nMC))                        # :64
        PB = np.zeros((Nf, G, nMC)) if phase else None     # :66 (all zeros without phase: not materialised then)
        absdot = np.zeros((Nf, G))                         # max over the draws of sum_v |z_v| |phi_v| (the tests' error scale)
        near_cut = np.zeros((Nf, G), dtype=bool)           # some draw sits within 1e-9 of the branch cut of angle
        for j in range(Nf):                                # :73
            zj = z[:, j::Nf]                               # :80  zi[iMC, j:Nf:end]
            dd = np.conj(zj) @ Kg.T                        # nMC x G
            FB[j] = np.abs(dd).T                           # :81
            absdot[j] = (np.abs(zj) @ np.abs(Kg).T).max(axis=0)
            if phase:
                PB[j] = np.angle(dd).T                     # :83
                near_cut[j] = (np.abs(PB[j]) > np.pi - 1e-9).any(axis=1)
        out["absdot"], out["dmin"], out["near_cut"] = absdot, FB.min(axis=2), near_cut
        FBs = np.sort(FB, axis=2)                          # :89
        lim = 10                                           # :90
        out["FBl"] = FBs[:, :, nMC // lim - 1]             # :91 (1-based nMC ÷ lim)
        out["FBu"] = FBs[:, :, nMC - nMC // lim - 1]       # :92
        out["FBm"] = FB.mean(axis=2)                       # :93
        if phase:
            PBs = np.sort(PB, axis=2)                      # :94
            out["PBl"] = PBs[:, :, nMC // lim - 1]         # :95
            out["PBu"] = PBs[:, :, nMC - nMC // lim - 1]   # :96
            out["PBm"] = PB.mean(axis=2)                   # :97
        else:
            out["PBl"] = out["PBu"] = out["PBm"] = np.zeros((Nf, G))
    nd = 0 if normdim == "freq" else 1                     # :99
    if normalization == "sum":                             # :101-102
        out["F"] = F / (F.sum(axis=nd, keepdims=True) / F.shape[nd])
    elif normalization == "max":                           # :103-104
        out["F"] = F / F.max(axis=nd, keepdims=True)       # :106 (F only: the bands are not normalised)
    return out


# ---- Philox4x32-10 and Box-Muller ---------------------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Ten rounds of Philox-4x32 on numpy uint64 arrays holding 32-bit words (Salmon et al. 2011, Fig. 2 / Random123 philox.h)."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) for c in ctr]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform_words(seed, rows, pairs):
    """The four 32-bit words behind the normals of (row i, column pair p) for every i in rows, p in pairs (arrays broadcast)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i, p = np.broadcast_arrays(np.asarray(rows, dtype=np.uint64), np.asarray(pairs, dtype=np.uint64))
    return philox4x32_10((i & np.uint64(MASK), i >> np.uint64(32), p & np.uint64(MASK), p >> np.uint64(32)), (seed & MASK, seed >> 32))


def box_muller(words, dtype=np.float64):
    """(z of column 2p, z of column 2p+1, radius) from the four words: 2 x 53 bits, u1 in (0, 1], angle 2 pi u2 as pi * t, t in [0, 2)."""
    w0, w1, w2, w3 = words
    a = ((w0 >> np.uint64(5)) << np.uint64(26)) | (w1 >> np.uint64(6))
    b = ((w2 >> np.uint64(5)) << np.uint64(26)) | (w3 >> np.uint64(6))
    u1 = (a + np.uint64(1)).astype(dtype) * dtype(2.0) ** -53
    t = b.astype(dtype) * dtype(2.0) ** -52
    r = np.sqrt(dtype(-2) * np.log(u1))
    # cospi / sinpi on the exact t: reduce to [-1/2, 1/2] exactly, then the plain functions at a small argument
    q = np.rint(t * 2)                                     # nearest multiple of 1/2 (exact)
    f = (t - q / 2) * dtype(np.pi) if dtype is np.float64 else (t - q / 2) * np.longdouble("3.14159265358979323846264338327950288")
    s, c = np.sin(f), np.cos(f)
    qi = q.astype(np.int64) % 4
    cs = np.choose(qi, [c, -s, -c, s])
    sn = np.choose(qi, [s, c, -s, -c])
    return r * cs, r * sn, r


def randn(seed, row0, rows, cols, dtype=np.float64):
    i = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    p = np.arange((cols + 1) // 2, dtype=np.uint64)[None, :]
    z0, z1, r = box_muller(uniform_words(seed, i, p), dtype)
    R = np.empty((rows, 2 * p.shape[1]), dtype=dtype)
    R[:, 0::2], R[:, 1::2] = z0, z1
    rad = np.repeat(r, 2, axis=1)
    return R[:, :cols], rad[:, :cols]


# ---- the test signal of test/runtests.jl:6-17 ----------------------------------------------------------------------------------------------
F_TRUE = [lambda v: 2 * v ** 2, lambda v: 2 / (5 * v + 1), lambda v: 3 * np.exp(-10 * (v - 0.5) ** 2)]   # test/runtests.jl:93


def generate_signal(f, w, N, modphase=False, seed=0):
    rng = np.random.default_rng(seed)                      # (Julia's stream is not reproduced: a fixed numpy seed)
    x = np.sort(10 * rng.random(N))                        # :7
    v = np.linspace(0, 1, N)                               # :8
    dep = np.stack([f[i % len(f)](v) for i in range(len(w))], axis=1)           # :12
    freq = np.cos(np.asarray(w)[None, :] * x[:, None] - 0.5 * modphase * dep)   # :13
    y = (dep * freq).sum(axis=1)                           # :14
    y = y + 0.1 * rng.standard_normal(N)                   # :15
    return y, v, x, freq, dep
