"""Host models of the packed inverse the ADMM mat-vec streams, numpy only: what every storage makes of
M = (G + I/mu)^-1, predicted bit for bit from the rounding rule of each format -- the GPU tests read the packed matrix back through
unit mat-vecs and compare entry by entry.

Conventions.  `A` is the inverse as the device holds it, row-major: A[r, c] = device M[r][c] (`Problem.get_inverse(shift).T`), n x n.
The device pads it to np = ceil(n/128)*128 with ones on the pad diagonal; the lower triangle is cut into 128 x 128 tiles
t = I(I+1)/2 + J (J <= I).  A tile below the diagonal serves both M[I, J] and, transposed, M[J, I]; a diagonal tile is used as it
stands (all 128 x 128 entries).  The model therefore returns the n x n matrix the product really multiplies, which is symmetric
across tiles whatever the bits of A's upper triangle are.

    f64    the doubles themselves
    f32    one rounding to float
    split  the 64-bit pattern rounded to nearest at bit 13, ties UP IN MAGNITUDE (add 2^12, clear the low 13 bits: the carry runs
           into the exponent); outside [2^-120, 2^127) a plain float
    mixed  per tile: fixed point -- value = clamp(rint(m / step), +-(2^35 - 1)) * step (rint: ties to even), step = 2^(e-35) per
           row with the row's max|m| < 2^e (a diagonal tile: without the diagonal, which is kept in doubles) -- iff every non-zero
           row has step <= 2^-44 max|M| sqrt(8192/np) and e - 35 >= -120, where max|M| is the largest diagonal entry OVER THE n
           VALID ROWS; otherwise `split`.  Diagonal tiles of ns > 1 handles are always `split`.  Fewer than half of all tiles
           fixed: the whole matrix is `split`.
    mixed32  the same tiles; the iteration reads 16 * (q >> 4) of the biased value q = rint(m / step) + 2^35, the nibbles q & 15
           (times step) form the matrix N = M36 - M32 of the stale nibble product
"""
import numpy as np

TS = 128
SPLIT_TILE_BYTES = 98304           # 128 x 128 x (4 + 2)
FIXED_TILE_BYTES = 74240           # 128 x 128 x 4 + 8192 of nibbles + 128 x 4 of steps
FIXED_DIAG_EXTRA = 1024            # the doubles of a fixed diagonal tile's diagonal
NIBBLE_BYTES = 8192
FLOAT_HEAD, FIXED, FIXED_DIAG = 0, 1, 2


def padded_size(n):
    return -(-int(n) // TS) * TS


def tile_list(np_):
    nb = np_ // TS
    return [(I, J) for I in range(nb) for J in range(I + 1)]


def split_round(a):
    """The 6-byte float-head element of every double of `a`, as a double."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    bits = a.view(np.uint64)
    r = ((bits + np.uint64(1 << 12)) & ~np.uint64((1 << 13) - 1)).view(np.float64)
    mag = np.abs(a)
    inside = (mag >= 2.0 ** -120) & (mag < 2.0 ** 127)
    with np.errstate(over="ignore"):
        return np.where(inside, r, a.astype(np.float32).astype(np.float64))


def split_ties(a):
    """Mask of the entries whose low 13 bits are exactly 2^12: the ties of `split_round`."""
    bits = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return (bits & np.uint64((1 << 13) - 1)) == np.uint64(1 << 12)


def row_steps(T, diagonal):
    """(step per row, exponent e per row) of one 128 x 128 tile; all-zero rows get step 0."""
    mag = np.abs(T)
    if diagonal:
        mag = mag.copy()
        np.fill_diagonal(mag, 0.0)
    rmax = mag.max(axis=1)
    _, e = np.frexp(rmax)                          # rmax = f 2^e, 1/2 <= f < 1: rmax < 2^e
    e = e.astype(np.int64)
    step = np.where(rmax > 0, np.ldexp(1.0, np.clip(e - 35, -1070, 1000).astype(np.int32)), 0.0)
    return step, e, rmax


def admission_limit(absmax, np_):
    return 2.0 ** -44 * absmax * np.sqrt(8192.0 / np_)


def fixed_tile(T, diagonal):
    """(36-bit value, 32-bit value the iteration of mixed32 handles reads, nibble part) of a tile stored in fixed point."""
    step, _, _ = row_steps(T, diagonal)
    st = np.where(step > 0, step, 2.0 ** -100)[:, None]
    src = T.copy()
    if diagonal:
        np.fill_diagonal(src, 0.0)
    q = np.clip(np.rint(src / st), -(2.0 ** 35 - 1), 2.0 ** 35 - 1).astype(np.int64) + (1 << 35)
    v36 = (q - (1 << 35)).astype(np.float64) * st
    v32 = (((q >> 4) << 4) - (1 << 35)).astype(np.float64) * st
    nib = (q & 15).astype(np.float64) * st
    if diagonal:                                   # kept apart in doubles, added by every kernel in full
        d = np.diag(T).copy()
        np.fill_diagonal(v36, d)
        np.fill_diagonal(v32, d)
        np.fill_diagonal(nib, 0.0)
    return v36, v32, nib


def tile_admitted(T, diagonal, limit):
    step, e, rmax = row_steps(T, diagonal)
    nz = rmax > 0
    return bool(np.all(~nz | ((step <= limit) & (e - 35 >= -120))))


def pad_device(A, n, np_):
    P = np.zeros((np_, np_))
    P[:n, :n] = A
    for i in range(n, np_):
        P[i, i] = 1.0
    return P


def packed_model(A, n, ns=1, storage="mixed", absmax="valid"):
    """The matrix the product multiplies.  Returns a dict:
      Mt       n x n doubles (mixed32: the 36-bit values)
      M32, N   mixed32 only: what the iteration reads, and the nibble matrix (Mt = M32 + N)
      types    mixed / mixed32: one format per tile (FLOAT_HEAD, FIXED, FIXED_DIAG), None otherwise
      storage  the storage in effect ("split" when fewer than half of the tiles were admitted)
      bytes    the bytes of M one product streams
    `absmax` = "valid": max|M| over the n valid rows; "padded": over all np diagonal entries, the pad's ones included."""
    A = np.asarray(A, dtype=np.float64)
    assert A.shape == (n, n)
    np_ = padded_size(n)
    if np_ < 2048:                                 # full symmetric doubles whatever the option says
        return dict(Mt=A.copy(), types=None, storage="full", bytes=8 * np_ * np_)
    P = pad_device(A, n, np_)
    tiles = tile_list(np_)
    ntiles = len(tiles)
    elems = ntiles * TS * TS

    def assemble(fn):
        out = np.zeros((np_, np_))
        for I, J in tiles:
            T = fn(P[I * TS:(I + 1) * TS, J * TS:(J + 1) * TS], I, J)
            out[I * TS:(I + 1) * TS, J * TS:(J + 1) * TS] = T
            if I != J:
                out[J * TS:(J + 1) * TS, I * TS:(I + 1) * TS] = T.T
        return out[:n, :n]

    if storage == "f64":
        return dict(Mt=assemble(lambda T, I, J: T), types=None, storage="f64", bytes=8 * elems)
    if storage == "f32":
        return dict(Mt=assemble(lambda T, I, J: T.astype(np.float32).astype(np.float64)), types=None, storage="f32", bytes=4 * elems)
    if storage == "split":
        return dict(Mt=assemble(lambda T, I, J: split_round(T)), types=None, storage="split", bytes=6 * elems)
    assert storage in ("mixed", "mixed32"), storage
    d = np.abs(np.diag(P))
    amax = float(d[:n].max() if absmax == "valid" else d.max())
    limit = admission_limit(amax, np_)
    types = np.zeros(ntiles, dtype=np.int64)
    for t, (I, J) in enumerate(tiles):
        if I == J and ns > 1:
            continue
        if tile_admitted(P[I * TS:(I + 1) * TS, J * TS:(J + 1) * TS], I == J, limit):
            types[t] = FIXED_DIAG if I == J else FIXED
    nfixed = int(np.count_nonzero(types))
    if 2 * nfixed < ntiles:
        return dict(Mt=assemble(lambda T, I, J: split_round(T)), types=np.zeros(ntiles, dtype=np.int64), storage="split", bytes=6 * elems,
                    limit=limit, absmax=amax)
    tindex = {ij: t for t, ij in enumerate(tiles)}
    parts = {}
    for which in range(3):
        parts[which] = assemble(lambda T, I, J, w=which: (fixed_tile(T, I == J)[w] if types[tindex[(I, J)]] else
                                                           (split_round(T) if w < 2 else np.zeros_like(T))))
    nbytes = nfixed * FIXED_TILE_BYTES + int(np.count_nonzero(types == FIXED_DIAG)) * FIXED_DIAG_EXTRA + (ntiles - nfixed) * SPLIT_TILE_BYTES
    if storage == "mixed32":
        nbytes -= nfixed * NIBBLE_BYTES
    return dict(Mt=parts[0], M32=parts[1], N=parts[2], types=types, storage=storage, bytes=nbytes, limit=limit, absmax=amax)


def fixed_tile_steps(A, n, types):
    """Largest row step of every fixed-point tile of the map `types` (0 for the others): what DESIGN 4.1 bounds."""
    np_ = padded_size(n)
    P = pad_device(A, n, np_)
    out = np.zeros(len(types))
    for t, (I, J) in enumerate(tile_list(np_)):
        if types[t]:
            out[t] = row_steps(P[I * TS:(I + 1) * TS, J * TS:(J + 1) * TS], I == J)[0].max()
    return out


def one_launch_quantum(A, n, vmax):
    """The quantum of the one-launch iteration's first launch after a state was set (header of csrc/admm_one_launch.hip):
    q = 2^(e-62), R V (1 + 1e-6) < 2^e, R the largest absolute row sum of M over the valid rows, V = (max|xb| + mu max|rhs|) / mu
    (`vmax`)."""
    R = float(np.abs(np.asarray(A)[:n, :n]).sum(axis=1).max())
    B = R * vmax * 1.000001
    _, e = np.frexp(max(B, 2.0 ** -900))
    return float(np.ldexp(1.0, int(e) - 62))
