"""Host mirror of the reference's estimator API on top of the HIP library.

Same names, argument order, keyword names (``λ``, ``μ``, ``proxg``, ``iters``, ``tol``,
``printerval``, ``cb``, ``init``, ``normalize``, ``coulomb``, ``nw``, ``noverlap``,
``window_func``, ``estimator``) and error behaviour as ``src/lsfft.jl`` / ``src/lasso.jl`` of
LPVSpectral.jl, so the parity tests read like ``test/runtests.jl``.  All arithmetic happens in
``liblpvspectral.so``; inputs may be numpy arrays (host) or float64 torch CUDA tensors (resident
in HBM).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import logging
import sys
from dataclasses import dataclass
from typing import Any, Callable, Optional

import numpy as np

from . import _lib
from ._lib import as_f32, is_f32, as_f64, check, lib, out_ptr
from .prox import IndBallL0, LeastSquares, NormL0, NormL1, NormL2, Quadratic, SlicedSeparableSum
from .windows import Windows2, Windows3, hanning, rect

log = logging.getLogger("lpvspectral")


# --------------------------------------------------------------------------- result type
@dataclass
class SpectralExt:
    """src/LPVSpectral.jl:59-70."""
    Y: Any
    X: Any
    V: Any
    w: Any
    Nv: int
    λ: float
    coulomb: bool
    normalize: bool
    x: Any
    Σ: Any


def abs2(x):
    """Julia's ``abs2``: re² + im² (not hypot²), so that e.g. ``ls_cohere(y,y) == 1`` holds exactly."""
    x = np.asarray(x)
    return x.real * x.real + x.imag * x.imag if np.iscomplexobj(x) else x * x


def _mul_conj(a, b):
    """``a .* conj.(b)`` evaluated as Julia does (four real products, no fused multiply-add): numpy's own complex multiply may
    contract to FMAs on some CPUs, and then ``ls_cohere(y, y) == 1`` (test/runtests.jl:207-208) holds only approximately."""
    a, b = np.asarray(a), np.asarray(b)
    ar, ai, br, bi = a.real, a.imag, b.real, b.imag
    return (ar * br + ai * bi) + 1j * (ai * br - ar * bi)


def reshape_params(x, Nf):
    """src/utilities.jl:77: params as an [Nω × Nv] matrix."""
    return np.reshape(np.asarray(x), (int(Nf), -1), order="F")


def psd(se: SpectralExt):
    """src/lsfft.jl:214-217."""
    rp = reshape_params(np.array(se.x, copy=True), len(np.ravel(se.w)))
    return abs2(rp.sum(axis=1, keepdims=True))


# --------------------------------------------------------------------------- small host helpers
def default_freqs(t_or_n, fs=None, n=None):
    """src/lsfft.jl:3-9: ``default_freqs(n::Int, fs=1)``, ``default_freqs(t)``, ``default_freqs(t, n)``.
    rfftfreq(n, fs) = (0:n÷2)·fs/n (host side, no FFTW)."""
    if np.isscalar(t_or_n):
        nn = int(t_or_n)
        fs = 1.0 if fs is None else float(fs)
    else:
        t32 = is_f32(t_or_n)
        t = _host(t_or_n)
        if n is not None:
            t = t[: int(n)]
        nn = len(t)
        if fs is None:
            fs = 1.0 / np.mean(np.diff(t))
        if t32:   # Float32 time stamps give a Float32 grid (rfftfreq(n, fs::Float32)): multiplier fs / n rounded to Float32, k * multiplier
            m = np.float32(np.float32(fs) / np.float32(nn))
            return (np.arange(nn // 2 + 1) * np.float64(m)).astype(np.float32)
    return (np.arange(nn // 2 + 1) * float(fs)) / nn


def _all_f32(*arrays):
    """Julia's eltype promotion for the entry points that take several arrays: Float32 only when every array is."""
    return all(is_f32(a) for a in arrays)


def _host_vec(a):
    """A host vector in its own float eltype (float32 stays float32: eltype promotion is decided later), anything else float64."""
    if is_f32(a) and not _lib.is_device_array(a):
        return np.ravel(np.asarray(a.detach().numpy() if hasattr(a, "detach") else a, dtype=np.float32))
    return np.ravel(_host(a))


def _host(a):
    if _lib.is_device_array(a):
        return a.detach().cpu().numpy().astype(np.float64, copy=False)
    if hasattr(a, "detach") and hasattr(a, "numpy"):
        a = a.detach().numpy()
    return np.asarray(a, dtype=np.float64)


def check_freq(f):
    """src/lsfft.jl:20-24 -> ``None`` or 1; ValueError (ArgumentError) if zero is not first."""
    z = C.c_int64(0)
    if is_f32(f):
        kf, pf, Nf = as_f32(f)
        check(lib().lpvs_check_freq_f32(pf, Nf, C.byref(z)))
    else:
        fa = np.ascontiguousarray(_host(f))
        check(lib().lpvs_check_freq_f64(out_ptr(fa), len(fa), C.byref(z)))
    return None if z.value == 0 else int(z.value)


def get_fourier_regressor(t, f):
    """src/lsfft.jl:26-49 -> ``(A, zerofreq)`` with A an N×Nreg column-major numpy array."""
    f32 = _all_f32(t, f)                              # t and f share the eltype T of src/lsfft.jl:26 (mixed: promoted to Float64 here)
    conv = as_f32 if f32 else as_f64
    kt, pt, N = conv(t)
    kf, pf, Nf = conv(f)
    zf = check_freq(f)
    nreg = 2 * Nf - (1 if zf else 0)
    A = np.zeros((N, nreg), order="F", dtype=np.float32 if f32 else np.float64)
    z = C.c_int64(0)
    fn = lib().lpvs_fourier_regressor_f32 if f32 else lib().lpvs_fourier_regressor_f64
    check(fn(pt, N, pf, Nf, out_ptr(A), C.byref(z)))
    return A, zf


def basis_activation_func(V, Nv, normalize=True, coulomb=False):
    """src/utilities.jl:23-36.  The reference returns a closure K(v); this mirror returns the table of
    K evaluated at every V[n] (N × Nv, or N × 2Nv with coulomb), which is how the closure is used
    (src/lasso.jl:42-44)."""
    kv, pv, N = as_f64(V)
    nb = 2 * Nv if coulomb else Nv
    K = np.zeros((N, nb), order="F")
    check(lib().lpvs_basis_activation_f64(pv, N, int(Nv), int(bool(normalize)), int(bool(coulomb)), out_ptr(K)))
    return K


def lpv_regressor(X, V, w, Nv, normalize=True, coulomb=False, permuted=True):
    """Materialised Φ of src/lasso.jl:35-50 (tests / small problems; the solve never forms it)."""
    f32 = _all_f32(X, V, w)                           # the phases w .* X promote (src/lasso.jl:39): Float32 only for an all-Float32 call
    conv = as_f32 if f32 else as_f64
    kx, px, N = conv(X)
    kv, pv, _ = conv(V)
    kw, pw, Nf = conv(_host_vec(w) if not _lib.is_device_array(w) else w)
    nb = 2 * Nv if coulomb else Nv
    Phi = np.zeros((N, 2 * Nf * nb), order="F", dtype=np.float32 if f32 else np.float64)
    fn = lib().lpvs_lpv_regressor_f32 if f32 else lib().lpvs_lpv_regressor_f64
    check(fn(px, pv, N, pw, Nf, int(Nv), int(bool(normalize)), int(bool(coulomb)), int(bool(permuted)), out_ptr(Phi)))
    return Phi


def fourier2complex(x, zerofreq):
    """src/utilities.jl:62-73 (host formatting helper)."""
    x = _host(x)
    n = len(x) // 2
    if zerofreq is None:
        return x[:n] + 1j * x[n:]
    out = np.empty(n + 1, dtype=np.complex128)
    out[0] = x[0]
    out[1:] = x[1:n + 1] + 1j * x[n + 1:]
    return out


def _host_qr_ridge(A, y, lam):
    """``[A; λI] \\ [y; 0]`` by LAPACK on the host -- the reference's own route (``real_complex_bs`` / ``fourier_solve``,
    src/utilities.jl:49-60) for the cases the device normal equations reject as singular to working precision."""
    n = A.shape[1]
    return np.linalg.lstsq(np.vstack([A, lam * np.eye(n)]), np.concatenate([np.asarray(y, dtype=np.float64), np.zeros(n)]), rcond=None)[0]


# --------------------------------------------------------------------------- options (include/lpvspectral.h LPVS_OPT_*)
def set_default_option(name, value=None):
    """Thread-local default for handles created / batched-window calls made afterwards: ``set_default_option("storage", "f64")``;
    ``None`` returns to the library's own choice (which the environment variable of the same name may override)."""
    oid, vid = _lib.option_ids(name, value)
    check(lib().lpvs_set_default_option(oid, vid))


def get_default_option(name):
    oid, vals = _lib.OPTIONS[name]
    v = C.c_int32(0)
    check(lib().lpvs_get_default_option(oid, C.byref(v)))
    named = {i: k for k, i in vals.items()}
    if name in _lib._INT_OPTIONS:                                    # integer-valued options: the number itself (None = no explicit default)
        return named.get(int(v.value), int(v.value) if v.value != 0 else None)
    return named.get(int(v.value))


class default_options:
    """``with default_options(storage="f64", iteration="two"): ...`` -- the defaults inside the block, the previous ones after it."""

    def __init__(self, **opts):
        self.opts = {k: v for k, v in opts.items() if v is not None}

    def __enter__(self):
        self.prev = {k: get_default_option(k) for k in self.opts}
        for k, v in self.opts.items():
            set_default_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            set_default_option(k, v)


def _with_options(fn):
    """Estimator / driver decorator: option keywords apply, as thread defaults, to everything the call creates."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        with default_options(**_pop_options(kwargs)):
            return fn(*args, **kwargs)
    return wrapper


def _pop_options(kwargs):
    """The option keywords of an estimator call (``storage=``, ``iteration=``, ``gram_form=``, ``nt_loads=``, ``slot_sums=``:
    extensions, the reference has none of them) taken out of ``kwargs``."""
    return {k: kwargs.pop(k) for k in list(kwargs) if k in _lib.OPTIONS}


# --------------------------------------------------------------------------- device problem handle
class Problem:
    """Owner of one ``lpvs_problem`` handle (regressor + Gram resident on one MI355X)."""

    ns = 1   # signals sharing the regressor (lpv_multi, path)
    weighted = False   # fourier(..., W): the estimator runs it as the reference's as-written Quadratic (linear term of the other sign)
    f32 = False   # created from float32 inputs: float I/O, single-precision copy of M in the ADMM mat-vec

    def __init__(self, handle, kind):
        self._h = handle
        self.kind = kind
        n = C.c_int64(0)
        check(lib().lpvs_problem_size(self._h, C.byref(n)))
        self.n = int(n.value)

    # constructors -----------------------------------------------------------------------
    @classmethod
    def fourier(cls, y, t, f, W=None, device=0):
        # eltype as the reference promotes it: the 3-argument method evaluates the regressor in T = eltype(y) (``T.(t), T.(f)``,
        # src/lasso.jl:91); the weighted 4-argument method in the eltype of t and f themselves (src/lasso.jl:111 -> src/lsfft.jl:26),
        # so a Float32 record with Float64 time stamps is a Float64 problem there -- t is never rounded to 24 bits
        f32 = is_f32(y) if W is None else _all_f32(y, t, f)
        conv = as_f32 if f32 else as_f64
        ky, py, N = conv(y)
        kt, pt, Nt = conv(t)
        kf, pf, Nf = conv(f)
        kw, pw, Nw = conv(W)
        assert N == Nt, "y and t has to be the same length"
        assert W is None or Nw == N, "W has to be the same length as y"
        h = C.c_void_p()
        fn = lib().lpvs_problem_create_fourier_f32 if f32 else lib().lpvs_problem_create_fourier_f64
        check(fn(py, pt, N, pf, Nf, pw, int(device), C.byref(h)))
        p = cls(h, "fourier")
        p.Nf, p.f32, p.weighted = Nf, f32, W is not None
        return p

    @classmethod
    def lpv(cls, y, X, V, w, Nv, normalize=True, coulomb=False, device=0):
        # Y, X, V::AbstractVector{S} (src/lasso.jl:27); the phases w .* X are formed in the promoted type of w and X (:39), so the
        # Float32 entry points serve only an all-Float32 call -- anything else is widened exactly and runs as a Float64 problem
        f32 = _all_f32(y, X, V, w)
        conv = as_f32 if f32 else as_f64
        ky, py, N = conv(y)
        kx, px, Nx = conv(X)
        kv, pv, Nvv = conv(V)
        kw, pw, Nf = conv(w)
        assert N == Nx == Nvv, "y, X and V has to be the same length"
        h = C.c_void_p()
        fn = lib().lpvs_problem_create_lpv_f32 if f32 else lib().lpvs_problem_create_lpv_f64
        check(fn(py, px, pv, N, pw, Nf, int(Nv), int(bool(normalize)), int(bool(coulomb)), int(device), C.byref(h)))
        p = cls(h, "lpv")
        p.Nf, p.nb, p.f32 = Nf, (2 * Nv if coulomb else Nv), f32
        return p

    @classmethod
    def lpv_multi(cls, Y, X, V, w, Nv, normalize=True, coulomb=False, device=0):
        """``Y`` is N x ns (one column per signal / channel) sharing ``X, V, w``: one Gram, ns right-hand sides."""
        if _all_f32(Y, X, V, w) and not _lib.is_device_array(Y):   # an all-Float32 call: the _f32 entry point (float I/O, double arithmetic)
            Yh = np.asfortranarray(np.asarray(Y, dtype=np.float32))
            N, ns = Yh.shape
            kx, px, Nx = as_f32(np.asarray(X, dtype=np.float32))
            kv, pv, Nvv = as_f32(np.asarray(V, dtype=np.float32))
            kw, pw, Nf = as_f32(np.asarray(w, dtype=np.float32))
            assert N == Nx == Nvv, "Y, X and V has to have the same number of samples"
            h = C.c_void_p()
            check(lib().lpvs_problem_create_lpv_multi_f32(out_ptr(Yh), int(ns), px, pv, N, pw, Nf, int(Nv), int(bool(normalize)), int(bool(coulomb)),
                                                          int(device), C.byref(h)))
            p = cls(h, "lpv")
            p.Nf, p.nb, p.ns, p.f32 = Nf, (2 * Nv if coulomb else Nv), int(ns), True
            return p
        if _lib.is_device_array(Y):
            assert Y.dim() == 2
            ns, N = Y.shape[1], Y.shape[0]
            Yc = Y.t().contiguous()                 # column-major N x ns == row-major [ns][N]
            ky, py = Yc, C.c_void_p(Yc.data_ptr())
        else:
            Yh = np.asfortranarray(_host(Y))
            N, ns = Yh.shape
            ky, py = Yh, out_ptr(Yh)
        kx, px, Nx = as_f64(X)
        kv, pv, Nvv = as_f64(V)
        kw, pw, Nf = as_f64(w)
        assert N == Nx == Nvv, "Y, X and V has to have the same number of samples"
        h = C.c_void_p()
        check(lib().lpvs_problem_create_lpv_multi_f64(py, int(ns), px, pv, N, pw, Nf, int(Nv), int(bool(normalize)), int(bool(coulomb)), int(device), C.byref(h)))
        p = cls(h, "lpv")
        p.Nf, p.nb, p.ns = Nf, (2 * Nv if coulomb else Nv), int(ns)
        return p

    @classmethod
    def lpv_rows(cls, y, X, V, w, Nv, ranges, normalize=True, coulomb=False, device=0):
        """Partial problem over a ROW SHARD ``(y, X, V)`` of one signal: ``ranges`` =
        ``[min V, max V, max|V|, max|X|]`` over ALL rows.  Its Gram / rhs are partial sums; exchange them with
        :meth:`device_gram` + an all-reduce, then :meth:`gram_modified`."""
        f32 = _all_f32(y, X, V, w) and not _lib.is_device_array(y)       # an all-Float32 call: the _f32 entry point
        conv = as_f32 if f32 else as_f64
        ky, py, N = conv(np.asarray(y, dtype=np.float32) if f32 else y)
        kx, px, Nx = conv(np.asarray(X, dtype=np.float32) if f32 else X)
        kv, pv, Nvv = conv(np.asarray(V, dtype=np.float32) if f32 else V)
        kw, pw, Nf = conv(np.asarray(w, dtype=np.float32) if f32 else w)
        assert N == Nx == Nvv, "y, X and V has to be the same length"
        r4 = np.ascontiguousarray(np.asarray(ranges, dtype=np.float64).ravel())
        assert r4.size == 4
        h = C.c_void_p()
        fn = lib().lpvs_problem_create_lpv_rows_f32 if f32 else lib().lpvs_problem_create_lpv_rows_f64
        check(fn(py, 1, px, pv, N, pw, Nf, int(Nv), int(bool(normalize)), int(bool(coulomb)), out_ptr(r4), int(device), C.byref(h)))
        p = cls(h, "lpv")
        p.Nf, p.nb = Nf, (2 * Nv if coulomb else Nv)
        p.f32 = f32
        return p

    @classmethod
    def dense(cls, A, y, W=None, device=0):
        if _lib.is_device_array(A):
            raise TypeError("dense(): pass A as a host (numpy) column-major matrix or a transposed-contiguous device tensor via gram()")
        Ah = np.asfortranarray(_host(A))
        m, n = Ah.shape
        ky, py, N = as_f64(y)
        kw, pw, Nw = as_f64(W)
        assert N == m
        h = C.c_void_p()
        check(lib().lpvs_problem_create_dense_f64(out_ptr(Ah), py, m, n, pw, int(device), C.byref(h)))
        return cls(h, "dense")

    @classmethod
    def gram(cls, G, b, device=0):
        kg, pg, n2 = as_f64(G)
        kb, pb, n = as_f64(b)
        assert n2 == n * n, "G must be n x n"
        h = C.c_void_p()
        check(lib().lpvs_problem_create_gram_f64(pg, pb, n, int(device), C.byref(h)))
        return cls(h, "gram")

    @classmethod
    def path(cls, src, ns):
        """A handle with ``ns`` signal slots from a single-signal problem of any constructor (extension): a device copy of ``src``'s Gram
        and ``ns`` copies of its right-hand side.  With a list of prox objects in :meth:`set_prox` the slots are ``ns`` penalties solved in
        one pass over one inverse.  ``src`` stays valid and independent."""
        h = C.c_void_p()
        check(lib().lpvs_problem_create_path(src._h, int(ns), C.byref(h)))
        p = cls(h, src.kind)
        for name in ("Nf", "nb"):
            if hasattr(src, name):
                setattr(p, name, getattr(src, name))
        p.ns, p.f32, p.weighted = int(ns), src.f32, src.weighted
        return p

    # housekeeping ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().lpvs_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # options --------------------------------------------------------------------------------
    def set_option(self, name, value=None):
        """``storage`` = "mixed" | "split" | "f64", ``iteration`` = "one" | "two", ``nt_loads`` = "on" | "off" (``None``: default);
        takes effect at the next :meth:`admm_init` / :meth:`admm_run`."""
        oid, vid = _lib.option_ids(name, value)
        check(lib().lpvs_problem_set_option(self._h, oid, vid))

    def get_option(self, name):
        """The value in effect for this handle (explicit, thread default or environment), ``None`` = the library's own choice."""
        oid, vals = _lib.OPTIONS[name]
        v = C.c_int32(0)
        check(lib().lpvs_problem_get_option(self._h, oid, C.byref(v)))
        return {i: k for k, i in vals.items()}.get(int(v.value))

    # accessors ------------------------------------------------------------------------------
    def get_gram(self):
        G = np.zeros((self.n, self.n), order="F")
        b = np.zeros(self.n)
        check(lib().lpvs_problem_get_gram_f64(self._h, out_ptr(G), out_ptr(b)))
        return G, b

    def get_rhs(self):
        b = np.zeros(self.n if self.ns == 1 else (self.n, self.ns), order="F")
        check(lib().lpvs_problem_get_rhs_f64(self._h, out_ptr(b)))
        return b

    def device_gram(self):
        """Torch views (no copy) of the handle's device Gram ``[np, np]`` and right-hand sides ``[ns, np]`` for an
        in-place exchange step; call :meth:`gram_modified` afterwards."""
        import torch
        G, b, npad = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        check(lib().lpvs_problem_device_gram_f64(self._h, C.byref(G), C.byref(b), C.byref(npad)))
        n_p = int(npad.value)

        class _View:   # __cuda_array_interface__ is how torch (CUDA and ROCm builds) adopts foreign device memory
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f8", "data": (int(ptr), False), "version": 3, "strides": None}

        dev = torch.device("cuda", torch.cuda.current_device())
        Gt = torch.as_tensor(_View(G.value, (n_p, n_p)), device=dev)
        bt = torch.as_tensor(_View(b.value, (self.ns, n_p)), device=dev)
        return Gt, bt

    def gram_modified(self):
        check(lib().lpvs_problem_gram_modified(self._h))

    def get_inverse(self, shift):
        M = np.zeros((self.n, self.n), order="F")
        check(lib().lpvs_problem_get_inverse_f64(self._h, float(shift), out_ptr(M)))
        return M

    def get_inverse_refined(self, shift):
        """``(G + shift I)⁻¹`` after one round of iterative refinement on the device (``lpvs_problem_get_inverse_refined_f64``), symmetrised:
        for an inverse that is itself the result.  :meth:`get_inverse` is the one the solves and the iteration apply."""
        M = np.zeros((self.n, self.n), order="F")
        check(lib().lpvs_problem_get_inverse_refined_f64(self._h, float(shift), out_ptr(M)))
        return 0.5 * (M + M.T)

    def solve_ridge(self, ridge):
        x = np.zeros(self.n, dtype=np.float32 if self.f32 else np.float64)
        fn = lib().lpvs_problem_solve_ridge_f32 if self.f32 else lib().lpvs_problem_solve_ridge_f64
        check(fn(self._h, float(ridge), out_ptr(x)))
        return x

    def set_prox(self, proxg):
        """One prox object for every signal, or a list / tuple of ``ns`` objects of one kind (and one group length): one per signal slot."""
        if isinstance(proxg, (list, tuple)):
            if not proxg or not all(hasattr(g, "device_params") for g in proxg):
                raise NotImplementedError("every entry of a per-signal proxg list must be a prox object with a device kernel")
            trip = [g.device_params(self.n) for g in proxg]
            if len({(k, gl) for k, _, gl in trip}) != 1:
                raise ValueError("the prox objects of a per-signal list must be of one kind and one group length")
            return self.set_prox_params(trip[0][0], [p for _, p, _ in trip], trip[0][2])
        if not hasattr(proxg, "device_params"):
            raise NotImplementedError(f"proxg of type {type(proxg).__name__} has no device kernel "
                                      "(supported: NormL1, NormL0, IndBallL0, SlicedSeparableSum(NormL2))")
        kind, param, glen = proxg.device_params(self.n)
        check(lib().lpvs_problem_set_prox(self._h, kind, float(param), int(glen)))

    def set_prox_params(self, kind, params, group_len=0):
        """``lpvs_problem_set_prox_per_signal``: prox ``kind`` (``_lib.PROX_*``) with ``params[q]`` for signal slot ``q`` (``ns`` values)."""
        pv = np.ascontiguousarray(np.asarray(params, dtype=np.float64).ravel())
        check(lib().lpvs_problem_set_prox_per_signal(self._h, int(kind), out_ptr(pv), int(pv.size), int(group_len)))

    def get_prox_params(self):
        """The parameter the prox of every signal slot will read (``ns`` values; the scalar repeated when one object is set)."""
        out = np.zeros(self.ns)
        check(lib().lpvs_problem_get_prox_params(self._h, out_ptr(out), int(out.size)))
        return out

    def admm_init(self, x0=None, μ=0.05, tol=1e-5, linear_sign=_lib.LINEAR_LEAST_SQUARES):
        k0, p0, n0 = (as_f32 if self.f32 else as_f64)(x0)
        assert x0 is None or n0 == self.n, "x0 has the wrong length"
        fn = lib().lpvs_admm_init_f32 if self.f32 else lib().lpvs_admm_init_f64
        check(fn(self._h, p0, float(μ), float(tol), int(linear_sign)))

    def admm_run(self, max_iters):
        it, nxz, conv = C.c_int64(0), C.c_double(0), C.c_int32(0)
        check(lib().lpvs_admm_run(self._h, int(max_iters), C.byref(it), C.byref(nxz), C.byref(conv)))
        return int(it.value), float(nxz.value), bool(conv.value)

    def admm_set_state(self, x, z, u, iters=0, offset=None):
        """Resume: install iterates saved by :meth:`admm_get` (after :meth:`admm_init` with the same parameters).  ``offset`` = the vector
        :meth:`admm_get_offset` returned with them (handles of n >= 2048): with it the run continues bit for bit, without it the library
        re-forms the vector from ``x`` (the same to second order)."""
        arrs = [np.asfortranarray(np.asarray(a, dtype=np.float32 if self.f32 else np.float64)) for a in (x, z, u)]
        assert all(a.size == self.n * self.ns for a in arrs), "x, z, u have the wrong length"
        fn = lib().lpvs_admm_set_state_f32 if self.f32 else lib().lpvs_admm_set_state_f64
        check(fn(self._h, out_ptr(arrs[0]), out_ptr(arrs[1]), out_ptr(arrs[2]), int(iters)))
        if offset is not None:
            off = np.asfortranarray(np.asarray(offset, dtype=np.float64))
            check(lib().lpvs_admm_set_offset_f64(self._h, out_ptr(off), int(off.size)))   # (a wrong length is the library's LPVS_EARGUMENT -> ValueError)

    def _offset_len(self):
        k = C.c_int64(0)
        check(lib().lpvs_admm_offset_len(self._h, C.byref(k)))
        return int(k.value)

    def admm_get_offset(self):
        """The offset vector of the x-update currently in effect (doubles), or ``None`` for handles without one (n < 2048).  Opaque:
        n x ns values, or 2 n for a handle that iterates on 32-bit reads of its fixed-point tiles (the vector with and without the nibble
        term of the last refresh; the first n are the offset the x-update adds)."""
        k = self._offset_len()
        if k == 0:
            return None
        xb = np.zeros(k if k != self.n * self.ns or self.ns == 1 else (self.n, self.ns), order="F")
        check(lib().lpvs_admm_get_offset_f64(self._h, out_ptr(xb), int(xb.size)))
        return xb

    def admm_get(self, f64=False):
        """``(x, z, u)`` in the handle's I/O type; ``f64=True``: the double state itself, of ``_f32`` handles too."""
        shape = self.n if self.ns == 1 else (self.n, self.ns)
        f32 = self.f32 and not f64
        x, z, u = (np.zeros(shape, order="F", dtype=np.float32 if f32 else np.float64) for _ in range(3))
        fn = lib().lpvs_admm_get_f32 if f32 else lib().lpvs_admm_get_f64
        check(fn(self._h, out_ptr(x), out_ptr(z), out_ptr(u)))
        return x, z, u

    def time_matvec(self, reps=200):
        """(microseconds per launch, bytes of M streamed per launch) of the ADMM mat-vec kernel, HIP events on the handle's stream."""
        us, nbytes = C.c_double(0), C.c_double(0)
        check(lib().lpvs_admm_time_matvec(self._h, int(reps), C.byref(us), C.byref(nbytes)))
        return float(us.value), float(nbytes.value)

    def matvec_info(self):
        """Kernel / storage of the inverse the ADMM mat-vec of this handle streams (after :meth:`admm_init`)."""
        k = C.c_int32(0)
        check(lib().lpvs_admm_matvec_kind(self._h, C.byref(k)))
        np_ = -(-self.n // 128) * 128
        one_launch = bool(int(k.value) & 16)
        fix32 = bool(int(k.value) & 32)            # the fixed-point tiles keep 32 significant bits (handles whose x-update is corrected)
        fixs = ("36-bit fixed point with per-row steps of which the iteration reads the 32 leading bits (4.03 B; the 4-bit planes meet a right-hand side "
                "every 32 iterations -- more often in the first 256 -- and ride in the offset vector: 32-bit fixed point reads)" if fix32 else
                "36-bit fixed point with per-row steps (4.53 B)")
        fixb = 66048 if fix32 else 74240
        k = C.c_int32(int(k.value) & 15)
        if one_launch and int(k.value) == 0:                               # small problems (np < 2048): full matrix, one launch per iteration
            return dict(kernel="admm_small_iter_kernel", one_launch_iteration=True,
                        storage="full symmetric f64; every workgroup redoes the update (prox, dual step, norm) and multiplies its four rows",
                        bytes_formula="8 B x np^2 (np = %d)" % np_)
        if one_launch and int(k.value) == 2:                               # _f32 handles: single-precision copy of the inverse
            return dict(kernel="admm_iter_mixed_kernel", one_launch_iteration=True,
                        storage="tile-packed lower triangle, f32 (4 B); tile partials added into x by 64-bit fixed-point atomics, prox / dual "
                                "update in the next launch's prologue",
                        bytes_formula="4 B x np(np+128)/2 (np = %d)" % np_)
        if one_launch:                                                     # mixed storage, single signal, fusable prox
            return dict(kernel="admm_iter_mixed_kernel", one_launch_iteration=True,
                        storage="tile-packed lower triangle, mixed: float head + 16-bit tail (6 B, 40 significant bits) for the diagonal tiles, "
                                + fixs + " for tiles of small entries; tile partials added into x by 64-bit "
                                "fixed-point atomics, prox / dual update in the next launch's prologue",
                        bytes_formula="98304 B per 6-byte tile, %d B per fixed-point tile (np = %d; 8-byte form %.1f MB)" % (fixb, np_, 8e-6 * np_ * (np_ + 128) / 2))
        if self.ns > 1 and int(k.value) == 4:                              # fixed-point tiles below the diagonal, float-head tiles on it
            q4 = self.ns <= 8 and os.environ.get("LPVS_MULTI_MFMA") != "16"
            nb = np_ // 128
            return dict(kernel="symv_tile_mfma_ws_kernel", storage="tile-packed lower triangle, mixed: 36-bit fixed point with per-row steps (4.53 B) for the "
                        "tiles below the diagonal, float head + 16-bit tail (6 B) for the diagonal tiles",
                        mfma="v_mfma_f64_4x4x4_4b_f64 (8 signal columns per pass, none padded)" if q4 else "v_mfma_f64_16x16x4_f64 (16 signal columns per pass)",
                        signals_per_pass=8 if q4 else 16,
                        bytes_formula="74240 B x %d tiles below the diagonal + 98304 B x %d diagonal tiles (np = %d), streamed once per %d signals"
                                      % (nb * (nb - 1) // 2, nb, np_, 8 if q4 else 16))
        if self.ns > 1 and int(k.value) in (1, 3):
            elt = 8 if int(k.value) == 1 else 6
            q4 = self.ns <= 8 and os.environ.get("LPVS_MULTI_MFMA") != "16"
            return dict(kernel="symv_tile_mfma_ws_kernel", storage="tile-packed lower triangle, %s" % ("f64 (8 B)" if elt == 8 else "float head + 16-bit tail (6 B, 40 significant bits)"),
                        mfma="v_mfma_f64_4x4x4_4b_f64 (8 signal columns per pass, none padded)" if q4 else "v_mfma_f64_16x16x4_f64 (16 signal columns per pass)",
                        signals_per_pass=8 if q4 else 16,
                        bytes_formula="%d B x np(np+128)/2 (np = %d), streamed once per %d signals" % (elt, np_, 8 if q4 else 16))
        return {0: dict(kernel="symv_kernel", storage="full symmetric f64", bytes_formula="8 B x np^2"),
                1: dict(kernel="symv_tile_kernel<double>", storage="tile-packed lower triangle, f64 (8 B)",
                        bytes_formula="8 B x np(np+128)/2 (np = %d)" % np_),
                2: dict(kernel="symv_tile_f32_kernel" if self.ns == 1 else "symv_tile_kernel<float>", storage="tile-packed lower triangle, f32 (4 B)",
                        bytes_formula="4 B x np(np+128)/2 (np = %d)" % np_),
                4: dict(kernel="symv_tile_mixed_kernel", storage="tile-packed lower triangle, mixed: float head + 16-bit tail (6 B, 40 significant bits) "
                                                                 "for the diagonal tiles, " + fixs + " for tiles of small entries",
                        bytes_formula="98304 B per 6-byte tile, %d B per fixed-point tile (np = %d; 8-byte form %.1f MB)" % (fixb, np_, 8e-6 * np_ * (np_ + 128) / 2)),
                3: dict(kernel="symv_tile_split_kernel", storage="tile-packed lower triangle, float head + 16-bit tail (6 B, 40 significant bits)",
                        bytes_formula="6 B x np(np+128)/2 (np = %d; the 8-byte form would be %.1f MB)" % (np_, 8e-6 * np_ * (np_ + 128) / 2))}[int(k.value)]

    def admm_status(self, signal=0):
        it, nxz, conv = C.c_int64(0), C.c_double(0), C.c_int32(0)
        check(lib().lpvs_admm_status(self._h, int(signal), C.byref(it), C.byref(nxz), C.byref(conv)))
        return int(it.value), float(nxz.value), bool(conv.value)

    def params(self, which=0):
        m = self.Nf * self.nb if self.kind == "lpv" else self.Nf
        shape = m if self.ns == 1 else (m, self.ns)
        dt = np.float32 if self.f32 else np.float64
        re, im = np.zeros(shape, order="F", dtype=dt), np.zeros(shape, order="F", dtype=dt)
        fn = lib().lpvs_problem_get_params_f32 if self.f32 else lib().lpvs_problem_get_params_f64
        check(fn(self._h, int(which), out_ptr(re), out_ptr(im)))
        return (re + 1j * im).astype(np.complex64 if self.f32 else np.complex128)

    def pack(self, coef):
        m = self.Nf * self.nb if self.kind == "lpv" else self.Nf
        kc, pc, _ = as_f64(coef)
        re, im = np.zeros(m), np.zeros(m)
        check(lib().lpvs_problem_pack_params_f64(self._h, pc, out_ptr(re), out_ptr(im)))
        return re + 1j * im

    def timing(self):
        t = np.zeros(15)
        check(lib().lpvs_problem_get_timing(self._h, out_ptr(t), 15))
        return dict(basis_ms=t[0], gram_ms=t[1], reduce_rhs_ms=t[2], factor_ms=t[3], admm_ms=t[4],
                    gram_issued_flops=t[5], gram_flops=t[6], admm_iters=t[7],
                    gram_form=("given", "kr", "krs", "panel", "ap", "ap-nufft")[int(t[8])],
                    xcorr_ms=t[9], xcorr_count=int(t[10]),      # the x-update corrections inside admm_ms
                    nibble_refreshes=int(t[11]), nibble_refresh_us=t[12],   # the stale nibble product's refreshes inside admm_ms; one of them, stand-alone
                    gram_stage=int(t[13]), gram_ksplit=int(t[14]))          # dense Gram: samples per stage of the gram_kernel instance, sample chunks (0: given / structured)


# --------------------------------------------------------------------------- ADMM driver
def _admm_on_problem(prob: Problem, x0, proxg, linear_sign, iters=10000, tol=1e-5, printerval=100, cb=None, μ=0.05,
                     out=sys.stdout):
    """src/lasso.jl:136-171 with the iterations on device.  Control returns to the host every
    ``printerval`` iterations, so the progress lines (:159,:165), ``cb(x,z)`` (:160-162) and
    KeyboardInterrupt (:59-63) behave as in the reference."""
    assert 0 <= μ <= 1, "μ should be ≤ 1"                       # src/lasso.jl:143
    prob.set_prox(proxg)
    prob.admm_init(x0, μ=μ, tol=tol, linear_sign=linear_sign)
    done, conv, nxz = 0, False, 0.0
    printerval = int(printerval) if printerval and printerval > 0 else iters
    while done < iters and not conv:
        chunk = min(printerval - done % printerval, iters - done)
        done, nxz, conv = prob.admm_run(chunk)
        if done % printerval == 0:
            print("%d ||x-z||₂ %.10f" % (done, nxz), file=out)      # src/lasso.jl:159
            if cb is not None:                                      # src/lasso.jl:160-162
                x, z, _ = prob.admm_get()
                cb(x, z)
        if conv:
            print("%d ||x-z||₂ %.10f" % (done, nxz), file=out)      # src/lasso.jl:165
            log.info("||x-z||₂ ≤ tol")                              # src/lasso.jl:166
            break
    x, z, _ = prob.admm_get()
    return x, z


def ADMM(x, proxf, proxg, iters=10000, tol=1e-5, printerval=100, cb=None, μ=0.05, device=0):
    """``ADMM(x, proxf, proxg; iters, tol, printerval, cb, μ)`` (src/lasso.jl:136-171) -> ``(x, z)``.

    ``proxf`` is a :class:`LeastSquares` (dense A, b) or :class:`Quadratic` (Q, q) mirror object; its
    Gram is formed / uploaded once and every iteration runs on the GPU."""
    if isinstance(proxf, LeastSquares):
        prob = Problem.dense(proxf.A, proxf.b, device=device)
    elif isinstance(proxf, Quadratic):
        prob = Problem.gram(proxf.Q, proxf.q, device=device)
    else:
        raise NotImplementedError(f"proxf of type {type(proxf).__name__} has no device path")
    with prob:
        return _admm_on_problem(prob, x, proxg, proxf.linear_sign, iters, tol, printerval, cb, μ)


# --------------------------------------------------------------------------- estimators
def ls_spectral(y, t, f=None, W=None, λ=1e-10, verbose=False, device=0):
    """``ls_spectral(y,t,f=default_freqs(t); λ=1e-10)`` (src/lsfft.jl:62-67) and the weighted
    ``ls_spectral(y,t,f,W; λ)`` (:74-80) -> ``(x, f)``.

    The weighted form is the reference's own formula ``(A'WA + λI) \\ A'Wy`` on the device Gram.  The
    unweighted form ``[A; λI] \\ [y; 0]`` is solved from normal equations in the better-conditioned shape:
    primal ``(A'A+λ²I)⁻¹A'y`` for tall systems, dual ``A'(AA'+λ²I)⁻¹y`` for fat ones (the reference's default
    frequency grid on an even-length record has one more column than rows) -- identical minimiser, no SVD."""
    f = default_freqs(t) if f is None else f
    if W is None:
        f32 = _all_f32(y, t, f)                                      # get_fourier_regressor(t, f) in their own eltype, src/lsfft.jl:63
        conv = as_f32 if f32 else as_f64
        ky, py, N = conv(y)
        kt, pt, Nt = conv(t)
        kf, pf, Nf = conv(f)
        assert N == Nt, "y and t has to be the same length"
        dt = np.float32 if f32 else np.float64
        re, im = np.zeros(Nf, dtype=dt), np.zeros(Nf, dtype=dt)
        fn = lib().lpvs_ls_spectral_f32 if f32 else lib().lpvs_ls_spectral_f64
        try:
            check(fn(py, pt, N, pf, Nf, float(λ), int(device), out_ptr(re), out_ptr(im)))
        except _lib.NumericError as e:
            # the normal equations (primal or dual) are singular to working precision -- irregular stamps on a grid they cannot resolve with
            # the default λ: the reference's QR of [A; λI] still works there.  Same route as ls_spectral_lpv, host LAPACK, on the regressor
            # the device kernel materialises (src/utilities.jl:55-60).
            log.info("ls_spectral: %s; solving [A; λI] \\ [y; 0] by QR on the host", e)
            A, zf = get_fourier_regressor(t, f)
            c = fourier2complex(_host_qr_ridge(np.asarray(A, dtype=np.float64), _host(y), float(λ)), zf)
            re, im = c.real.astype(dt), c.imag.astype(dt)
        if verbose:                                                 # src/lsfft.jl:65: cond(A'A), from the device Gram
            with Problem.fourier(y, t, f, None, device=device) as prob:
                G, _ = prob.get_gram()
            log.info("Condition number: %s\n", round(float(np.linalg.cond(G)), 2))
        return (re + 1j * im).astype(np.complex64 if f32 else np.complex128), _host(f)
    with Problem.fourier(y, t, f, W, device=device) as prob:
        x = prob.solve_ridge(λ)
        if verbose:
            G, _ = prob.get_gram()
            log.info("Condition number: %s\n", round(float(np.linalg.cond(G)), 2))
        params = prob.pack(x)
    return params, _host(f)


def tls_spectral(y, t, f=None, device=0):
    """``tls_spectral(y,t,f=default_freqs(t)[1:end-1])`` (src/lsfft.jl:85-99) -> ``(x, f)``: total least squares.

    The reference takes the right singular vector of the smallest singular value of ``[A y]``; it is the eigenvector of
    the smallest eigenvalue of ``[A y]'[A y] = [[A'A, A'y], [y'A, y'y]]``.  The O(N n²) part -- ``A'A`` and ``A'y`` -- is
    the device Gram of the Fourier problem; the (n+1)×(n+1) symmetric eigenproblem goes to the host LAPACK, as the
    reference's own ``LAPACK.gesvd!`` does."""
    f = default_freqs(t)[:-1] if f is None else f
    yh = _host(y).astype(np.float64)
    with Problem.fourier(y, t, f, None, device=device) as prob:
        G, b = prob.get_gram()
        n = prob.n
        H = np.empty((n + 1, n + 1))
        H[:n, :n] = G
        H[:n, n] = b
        H[n, :n] = b
        H[n, n] = float(np.dot(yh, yh))
        _, V = np.linalg.eigh(H)
        v = V[:, 0]                                                  # smallest eigenvalue first
        params = prob.pack(-v[:n] / v[n])                            # x = -V21 / V22, fourier2complex
    return params, _host(f)


def ls_sparse_spectral(y, t, f=None, W=None, init=False, λ=1.0, proxg=None, device=0, **kwargs):
    """``ls_sparse_spectral(y,t,f; init, λ, proxg=NormL1(λ), kwargs...)`` (src/lasso.jl:85-102) and the
    weighted 4-argument method ``(y,t,f,W; ...)`` (:105-126) -> ``(params, f)``.

    The weighted method reproduces the reference as written: ``Quadratic(Q, q=+A'Wy)``
    (src/lasso.jl:119-121), i.e. the linear term enters with the opposite sign of least squares."""
    f = default_freqs(t) if f is None else f
    proxg = NormL1(λ) if proxg is None else proxg
    with default_options(**_pop_options(kwargs)), Problem.fourier(y, t, f, W, device=device) as prob:
        x0 = None
        if init:  # fourier_solve(A,y,zerofreq,λ), src/lasso.jl:92,112 -- UNWEIGHTED in both methods (:112 ignores W)
            zf = check_freq(f)
            if W is None:
                p = prob.pack(prob.solve_ridge(λ * λ))               # the handle's own Gram is the unweighted one
            else:
                p = ls_spectral(y, t, f, λ=λ, device=device)[0]
            p = np.asarray(p, dtype=np.complex128)
            x0 = np.concatenate([p.real, p.imag[1:] if zf else p.imag])  # src/lasso.jl:93-97
        sign = _lib.LINEAR_LEAST_SQUARES if W is None else _lib.LINEAR_QUADRATIC_AS_WRITTEN
        _admm_on_problem(prob, x0, proxg, sign, **kwargs)
        params = prob.params(0)                                      # fourier2complex(z, zerofreq)
    return params, _host(f)


def ls_sparse_spectral_lpv(y, X, V, w, Nv, λ=1, coulomb=False, normalize=True, device=0, proxg=None, **kwargs):
    """``ls_sparse_spectral_lpv(Y,X,V,w,Nv; λ, coulomb, normalize, kwargs...)`` (src/lasso.jl:27-70)
    -> :class:`SpectralExt` with ``Σ=None``.

    ``proxg=None`` gives the reference's frequency-grouped lasso (src/lasso.jl:53-55); passing another
    prox object (e.g. ``IndBallL0(32)``) is an extension the reference does not have."""
    if coulomb:
        raise NotImplementedError("coulomb=true is ill-defined in the reference's sparse LPV path "
                                  "(half of x is never written by prox!, SURVEY.md §2 ‡); use ls_spectral_lpv")
    w = _host_vec(w) if not _lib.is_device_array(w) else w
    Nf = len(w)
    Nv = int(Nv)
    with default_options(**_pop_options(kwargs)), Problem.lpv(y, X, V, w, Nv, normalize, False, device=device) as prob:
        g = SlicedSeparableSum.frequency_groups(λ, Nf, 2 * Nv) if proxg is None else proxg
        try:
            _admm_on_problem(prob, None, g, _lib.LINEAR_LEAST_SQUARES, **kwargs)
            params = prob.params(0)
        except KeyboardInterrupt:                                    # src/lasso.jl:59-63
            log.info("Aborting")
            params = prob.params(1)                                  # z = copy(x)
    return SpectralExt(y, X, V, w, Nv, λ, coulomb, normalize, params, None)


# --------------------------------------------------------------------------- regularisation paths (extension)
def lambda_max(prob, proxg_kind, group_len=0):
    """The smallest penalty whose solution is all-zero, from the handle's right-hand side ``b = A'y``: the KKT conditions of
    ``½‖Ax−y‖² + λ g(x)`` at ``x = 0`` are ``‖b‖∞ ≤ λ`` for ``NormL1`` and ``max_g ‖b_g‖₂ ≤ λ`` for the grouped lasso (contiguous groups of
    ``group_len``).  ``proxg_kind``: a prox class, object or ``_lib.PROX_*`` id.  ``NormL0`` / ``IndBallL0`` have no such value, and the
    weighted Fourier problem runs as the reference's as-written ``Quadratic``, whose linear term has the other sign: ``ValueError``.
    A handle with several signals gives one value per signal."""
    kind = getattr(proxg_kind, "kind", proxg_kind)
    if kind not in (_lib.PROX_L1, _lib.PROX_GROUP_L2):
        raise ValueError("lambda_max is defined for NormL1 and the grouped lasso only (NormL0 / IndBallL0 have no penalty that gives x = 0)")
    if getattr(prob, "weighted", False):
        raise ValueError("lambda_max: the weighted problem is the as-written Quadratic (linear term of the other sign), not ½‖Ax−y‖²")
    B = np.abs(np.asarray(prob.get_rhs(), dtype=np.float64).reshape(prob.n, -1, order="F"))
    if kind == _lib.PROX_GROUP_L2:
        gl = int(group_len or getattr(proxg_kind, "group_len", 0))
        if gl <= 0:
            raise ValueError("lambda_max of the grouped lasso needs group_len > 0")
        ng = prob.n // gl
        out = np.sqrt((B[:ng * gl] ** 2).reshape(ng, gl, -1).sum(axis=1)).max(axis=0)
    else:
        out = B.max(axis=0)
    return float(out[0]) if out.size == 1 else out


def lambda_grid(lmax, count, ratio=1e-3):
    """``count`` penalties, geometric from ``lmax`` down to ``ratio·lmax`` (both end points exact; ``count = 1``: ``[lmax]``)."""
    count = int(count)
    if count < 1 or not (lmax > 0) or not (0 < ratio <= 1):
        raise ValueError("lambda_grid needs count >= 1, lmax > 0 and 0 < ratio <= 1")
    if count == 1:
        return np.array([float(lmax)])
    return float(lmax) * float(ratio) ** (np.arange(count) / (count - 1.0))


def _path_proxgs(src, λs, nλ, proxg, make, kind, group_len):
    """The prox objects of a path and the value each stands for: ``proxg`` (a list, e.g. ``[IndBallL0(4), IndBallL0(8)]``) as given, else
    ``make(λ)`` over ``λs`` (``None``: ``lambda_grid(lambda_max(src, ...), nλ)``)."""
    if proxg is not None:
        gs = list(proxg)
        return gs, np.array([float(g.device_params(src.n)[1]) for g in gs])
    if λs is None:
        λs = lambda_grid(lambda_max(src, kind, group_len), nλ)
    λs = np.asarray(λs, dtype=np.float64).ravel()
    return [make(l) for l in λs], λs


def ls_sparse_spectral_path(y, t, f=None, W=None, λs=None, nλ=8, proxg_kind=NormL1, **kwargs):
    """:func:`ls_sparse_spectral` for a whole regularisation path (extension) -> ``(params[Nf, nλ], f, λs)``: column ``q`` is the estimate
    with ``proxg_kind(λs[q])``.  One Gram, one factorisation and one pass over the inverse per iteration serve every penalty; each column
    stops at its own ``‖x−z‖₂ < tol``.  ``λs=None``: ``lambda_grid(lambda_max(...), nλ)``; ``proxg=[IndBallL0(4), IndBallL0(8), …]``
    gives an ``r``-path (``λs`` returned: the ``r``); ``group_len=`` with ``proxg_kind=SlicedSeparableSum``."""
    f = default_freqs(t) if f is None else f
    device, proxg, gl = kwargs.pop("device", 0), kwargs.pop("proxg", None), int(kwargs.pop("group_len", 0))
    with default_options(**_pop_options(kwargs)):
        with Problem.fourier(y, t, f, W, device=device) as src:
            make = (lambda l: SlicedSeparableSum.frequency_groups(l, src.n // gl, gl)) if proxg_kind is SlicedSeparableSum else proxg_kind
            gs, vals = _path_proxgs(src, λs, nλ, proxg, make, proxg_kind, gl)
            prob = Problem.path(src, len(gs))
        with prob:
            sign = _lib.LINEAR_LEAST_SQUARES if W is None else _lib.LINEAR_QUADRATIC_AS_WRITTEN
            _admm_on_problem(prob, None, gs, sign, **kwargs)
            params = prob.params(0).reshape(prob.Nf, -1, order="F")
    return params, _host(f), vals


def ls_sparse_spectral_lpv_path(y, X, V, w, Nv, λs=None, nλ=8, proxg=None, normalize=True, **kwargs):
    """:func:`ls_sparse_spectral_lpv` for a whole regularisation path (extension) -> a list of :class:`SpectralExt`, one per penalty of
    the frequency-grouped lasso, each with its own ``λ``.  Rules as :func:`ls_sparse_spectral_path`."""
    w = _host_vec(w) if not _lib.is_device_array(w) else w
    Nf, Nv = len(w), int(Nv)
    device = kwargs.pop("device", 0)
    with default_options(**_pop_options(kwargs)):
        with Problem.lpv(y, X, V, w, Nv, normalize, False, device=device) as src:
            gs, vals = _path_proxgs(src, λs, nλ, proxg, lambda l: SlicedSeparableSum.frequency_groups(l, Nf, 2 * Nv), SlicedSeparableSum, 2 * Nv)
            prob = Problem.path(src, len(gs))
        with prob:
            _admm_on_problem(prob, None, gs, _lib.LINEAR_LEAST_SQUARES, **kwargs)
            P = prob.params(0).reshape(Nf * Nv, -1, order="F")
    return [SpectralExt(y, X, V, w, Nv, float(vals[q]), False, normalize, P[:, q].copy(), None) for q in range(len(gs))]


def lpv_ranges(X, V):
    """``[min V, max V, max|V|, max|X|]`` of a (shard of a) signal, reduced on the device."""
    kx, px, N = as_f64(X)
    kv, pv, Nv_ = as_f64(V)
    assert N == Nv_
    out = np.zeros(4)
    check(lib().lpvs_lpv_ranges_f64(px, pv, N, out_ptr(out)))
    return out


# --------------------------------------------------------------------------- model evaluation (extension)
_EVAL_PATHS = {"auto": 0, "direct": 1, "nufft": 2}


def _f64_arg(a):
    """float32 inputs are widened (device tensors on the device, everything else on the host)."""
    if a is not None and _lib.is_device_array(a) and is_f32(a):
        return a.double()
    return a


def _coef_columns(x, n):
    """Coefficients as an (n, nc) complex column-major matrix and whether the caller gave a single vector."""
    P = np.asarray(_host_c(x) if np.iscomplexobj(np.asarray(x)) else _host(x))
    single = P.ndim == 1
    P = P.reshape(P.shape[0], -1)
    if P.shape[0] != n:
        raise ValueError(f"{P.shape[0]} coefficients per column, the model has {n}")
    return np.asfortranarray(P.astype(np.complex128)), single


def _evaluate(se, a, b, y, path, device, out, want_sums):
    """Shared by predict / residual / fva -> (output, sums or None, M).  ``se``: a :class:`SpectralExt` (``a``, ``b`` = X, V or None)
    or Fourier coefficients (``a``, ``b`` = f, t)."""
    if path not in _EVAL_PATHS:
        raise ValueError(f"path: unknown value {path!r} (known: {sorted(_EVAL_PATHS)})")
    lpv = isinstance(se, SpectralExt)
    if lpv:
        w = np.ascontiguousarray(_host_vec(se.w).astype(np.float64))
        Nf, Nv = len(w), int(se.Nv)
        nb = 2 * Nv if se.coulomb else Nv
        P, single = _coef_columns(se.x, Nf * nb)
        X = _f64_arg(se.X if a is None else a)
        V = _f64_arg(se.V if b is None else b)
        ranges = np.ascontiguousarray(lpv_ranges(_f64_arg(se.X), _f64_arg(se.V))[:3])   # of the TRAINING record: the fitted basis
        kx, px, M = as_f64(X)
        kv, pv, Mv = as_f64(V)
        assert M == Mv, "X and V has to be the same length"
    else:
        if a is None or b is None:
            raise TypeError("predict(x, f, t): the frequencies and the sampling points are needed")
        f = np.ascontiguousarray(_host_vec(a).astype(np.float64))
        Nf = len(f)
        xa = np.asarray(se if not hasattr(se, "detach") else se.detach().cpu().numpy())
        if not np.iscomplexobj(xa) and xa.shape[0] != Nf:                # the real vector [cos; sin] the regressor multiplies
            zf = check_freq(f)
            cols = xa.reshape(xa.shape[0], -1)
            xa = np.stack([fourier2complex(cols[:, q], zf) for q in range(cols.shape[1])], axis=1).reshape((Nf,) + xa.shape[1:])
        P, single = _coef_columns(xa, Nf)
        kx, px, M = as_f64(_f64_arg(b))
    nc = P.shape[1]
    pre, pim = np.asfortranarray(P.real), np.asfortranarray(P.imag)
    ky, py, My = as_f64(_f64_arg(y))
    if y is not None:
        assert My == M, "y has to be as long as the sampling points"
    if out is None:
        res = np.zeros(M if single else (M, nc), order="F")
        po = out_ptr(res)
    else:
        ko, po, no = as_f64(out)
        if no != M * nc:
            raise ValueError(f"out has {no} elements, {M} x {nc} are written (column-major)")
        res = out
    sums = np.zeros(2 * nc) if want_sums else None
    ps = out_ptr(sums) if want_sums else None
    if lpv:
        check(lib().lpvs_lpv_eval_f64(out_ptr(pre), out_ptr(pim), nc, out_ptr(w), Nf, Nv, int(bool(se.normalize)), int(bool(se.coulomb)), out_ptr(ranges),
                                      px, pv, py, M, _EVAL_PATHS[path], int(device), po, ps))
    else:
        check(lib().lpvs_fourier_eval_f64(out_ptr(pre), out_ptr(pim), nc, out_ptr(f), Nf, px, py, M, _EVAL_PATHS[path], int(device), po, ps))
    return res, (sums.reshape(nc, 2) if want_sums else None), M, single


def predict(se, X=None, V=None, path="auto", device=0, out=None):
    """The fitted model at samples (extension; the reference has no predict), without materialising the regressor.

    ``predict(se, X=None, V=None)``: an LPV estimate (:class:`SpectralExt`) at its own samples or at new ``X``, ``V`` -- the basis is the
    FITTED one (centres from the ranges of ``se.V``), not a basis of the new ``V``; equals ``lpv_regressor(X, V, w, Nv, normalize,
    coulomb, permuted=False) @ [re x; im x]`` on the training record.  ``predict(x, f, t)``: a Fourier estimate (what ``ls_spectral``
    returns, or the real coefficient vector) at sampling points ``t``; equals ``get_fourier_regressor(t, f)[0] @ x``.
    Coefficients may be one vector or an (n, nc) matrix (a regularisation path): the result is (M,) or (M, nc), each column to the bits
    of its own call.  ``path``: ``"auto"``, ``"direct"`` (any frequency grid) or ``"nufft"`` (a type-2 non-uniform FFT for grids that
    are an arithmetic progression up to rounding; ValueError otherwise).  ``out``: a float64 array / device tensor of M·nc elements
    that is filled column-major and returned instead of a new numpy array."""
    return _evaluate(se, X, V, None, path, device, out, False)[0]


def residual(se, f=None, t=None, y=None, path="auto", device=0, out=None, return_sums=False):
    """``residual(se)`` = ``se.Y - predict(se)`` and ``residual(x, f, t, y)`` = ``y - predict(x, f, t)``, formed on the device (one
    column per coefficient column).  ``return_sums``: also the device's ``[Σe, Σe²]`` per column, an (nc, 2) array -- added in a fixed
    order, so two calls give the same bits."""
    if isinstance(se, SpectralExt):
        if f is not None or t is not None or y is not None:
            raise TypeError("residual(se) is taken at the fitted samples")
        y, f, t = se.Y, None, None
    elif y is None:
        raise TypeError("residual(x, f, t, y): the signal is needed")
    e, sums, _, _ = _evaluate(se, f, t, y, path, device, out, bool(return_sums))
    return (e, sums) if return_sums else e


def fva(se, f=None, t=None, y=None, path="auto", device=0):
    """Fraction of variance explained, ``1 - var(e) / var(y)`` with the corrected variances (src/lsfft.jl:255), for ``fva(se)`` or
    ``fva(x, f, t, y)``; one value per coefficient column for a path.  ``var(e)`` comes from the device's sums of ``e`` and ``e²``."""
    if isinstance(se, SpectralExt):
        if f is not None or t is not None or y is not None:
            raise TypeError("fva(se) is taken at the fitted samples")
        y, f, t = se.Y, None, None
    elif y is None:
        raise TypeError("fva(x, f, t, y): the signal is needed")
    _, sums, M, single = _evaluate(se, f, t, y, path, device, None, True)
    var_e = (sums[:, 1] - sums[:, 0] * sums[:, 0] / M) / (M - 1)
    r = 1.0 - var_e / float(np.var(_host(_f64_arg(y)), ddof=1))
    return float(r[0]) if single else r


def eval_last_timing():
    """Timing of the calling thread's last predict / residual / fva: the path taken, the fine grid, whether the first-order twin grids
    ran, milliseconds per phase and the slabs of partial sums."""
    t = np.zeros(10)
    check(lib().lpvs_eval_last_timing(out_ptr(t), 10))
    return {"path": {1: "direct", 2: "nufft"}.get(int(t[0]), "none"), "nf": int(t[1]), "twin": bool(t[2]), "stage_ms": float(t[3]), "grid_ms": float(t[4]),
            "eval_ms": float(t[5]), "sums_ms": float(t[6]), "copy_ms": float(t[7]), "total_ms": float(t[8]), "slabs": int(t[9])}


def ls_sparse_spectral_lpv_rowsharded(y, X, V, w, Nv, λ=1, normalize=True, device=0, proxg=None, dist=None, **kwargs):
    """One signal whose SAMPLE ROWS are sharded over the ranks of ``dist`` (``torch.distributed``, initialised;
    backend nccl = RCCL over xGMI): every rank passes its rows ``(y, X, V)``.  SURVEY.md §8(e)(2): each rank forms the
    partial Gram / rhs of its rows on its GPU, ONE all-reduce sums them (n_p² + n_p f64 per rank), and the ADMM
    (src/lasso.jl:136-171) then runs replicated, so every rank returns the same :class:`SpectralExt` as
    :func:`ls_sparse_spectral_lpv` on the whole signal (up to the summation order of the Gram)."""
    from . import sharding
    w = _host_vec(w) if not _lib.is_device_array(w) else w
    Nf, Nv = len(w), int(Nv)
    ranges = sharding.allreduce_ranges(lpv_ranges(X, V), dist)
    with Problem.lpv_rows(y, X, V, w, Nv, ranges, normalize, False, device=device) as prob:
        G, b = prob.device_gram()
        sharding.allreduce_sum_(G, dist)
        sharding.allreduce_sum_(b, dist)
        prob.gram_modified()
        g = SlicedSeparableSum.frequency_groups(λ, Nf, 2 * Nv) if proxg is None else proxg
        _admm_on_problem(prob, None, g, _lib.LINEAR_LEAST_SQUARES, **kwargs)
        params = prob.params(0)
    return SpectralExt(y, X, V, w, Nv, λ, False, normalize, params, None)


def ls_sparse_spectral_lpv_multi(Y, X, V, w, Nv, λ=1, normalize=True, device=0, proxg=None, **kwargs):
    """Batched multichannel form of :func:`ls_sparse_spectral_lpv` (extension; BASELINE.json config 5): the columns
    of ``Y`` (N x ns) are independent signals sharing ``X, V, w``.  One Gram / factorisation, every ADMM kernel
    advances all signals; each signal stops at its own ``‖x−z‖₂ < tol``.  Returns a list of :class:`SpectralExt`
    whose entries equal the single-signal results."""
    w = _host_vec(w) if not _lib.is_device_array(w) else w
    Nf, Nv = len(w), int(Nv)
    with default_options(**_pop_options(kwargs)), Problem.lpv_multi(Y, X, V, w, Nv, normalize, False, device=device) as prob:
        g = SlicedSeparableSum.frequency_groups(λ, Nf, 2 * Nv) if proxg is None else proxg
        _admm_on_problem(prob, None, g, _lib.LINEAR_LEAST_SQUARES, **kwargs)
        P = prob.params(0)
        ns = prob.ns
    P = P.reshape(-1, ns, order="F")
    Yh = Y if not _lib.is_device_array(Y) else None
    return [SpectralExt(None if Yh is None else np.asarray(Yh)[:, q], X, V, w, Nv, λ, False, normalize, P[:, q].copy(), None)
            for q in range(ns)]


def lpv_batch_multi(Y, X, V, w, Nv, proxg=None, λ=1, normalize=True, μ=0.05, tol=1e-5, iters=10000, ngpus=0, devices=None):
    """``lpvs_lpv_batch_multi_f64``: the channels (columns of ``Y``, N x ns) split into contiguous ranges over ``ngpus`` devices driven
    by this one process (a host thread per device: one Gram / factorisation per device, its channels advanced together).  Returns
    ``(params [Nf*Nv x ns complex], iters [ns])``; no progress lines / callbacks (use :func:`ls_sparse_spectral_lpv_multi` per device
    for those)."""
    assert 0 <= μ <= 1, "μ should be ≤ 1"                             # src/lasso.jl:143
    w = _host_vec(w).astype(np.float64)
    Yh = np.asfortranarray(_host(Y))
    N, ns = Yh.shape
    Xh, Vh = np.ascontiguousarray(_host(X)), np.ascontiguousarray(_host(V))
    assert N == len(Xh) == len(Vh), "Y, X and V has to have the same number of samples"
    Nf, Nv = len(w), int(Nv)
    g = SlicedSeparableSum.frequency_groups(λ, Nf, 2 * Nv) if proxg is None else proxg
    kind, param, glen = g.device_params(2 * Nf * Nv)
    dv = None if devices is None else np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
    if dv is not None:
        ngpus = len(dv)
    m = Nf * Nv
    re, im = np.zeros((m, ns), order="F"), np.zeros((m, ns), order="F")
    its = np.zeros(ns, dtype=np.int64)
    check(lib().lpvs_lpv_batch_multi_f64(out_ptr(Yh), ns, out_ptr(Xh), out_ptr(Vh), N, out_ptr(w), Nf, Nv, int(bool(normalize)), int(kind), float(param),
                                         int(glen), float(μ), float(tol), int(iters), None if dv is None else out_ptr(dv), int(ngpus),
                                         out_ptr(re), out_ptr(im), out_ptr(its)))
    return re + 1j * im, its


def lpv_signals_multi(Y, X, V, w, Nv, proxg=None, λ=1, normalize=True, μ=0.05, tol=1e-5, iters=10000, ngpus=0, devices=None, in_flight=2):
    """``lpvs_lpv_signals_multi_f64``: the loop ``[ls_sparse_spectral_lpv(Y[:, q], X[:, q], V[:, q], w, Nv; ...) for q]`` inside the
    library -- every signal its own samples of X and V (all three N x nsig), contiguous signal ranges over ``ngpus`` devices,
    ``in_flight`` solves at a time per device (each on its own handle and stream).  Returns ``(params [Nf*Nv x nsig complex],
    iters [nsig])``; the results do not depend on ``ngpus`` / ``in_flight``."""
    assert 0 <= μ <= 1, "μ should be ≤ 1"                             # src/lasso.jl:143
    w = _host_vec(w).astype(np.float64)
    dev_in = all(_lib.is_device_array(a) for a in (Y, X, V))
    if dev_in:                                                        # resident inputs (column-major N x nsig on the device) are used in place
        import torch
        if not all(a.dtype == torch.float64 for a in (Y, X, V)):     # the _f64 entry point reads 8-byte elements: never reinterpret
            raise TypeError("lpv_signals_multi: device inputs must be float64 tensors (got %s)" % ", ".join(str(a.dtype) for a in (Y, X, V)))
        if not (Y.device == X.device == V.device):
            raise ValueError("lpv_signals_multi: Y, X and V must live on the same device (got %s, %s, %s)" % (Y.device, X.device, V.device))
        if Y.dim() != 2:
            raise ValueError("lpv_signals_multi: device inputs are N x nsig matrices")
        Yh, Xh, Vh = Y, X, V
        N, nsig = int(Y.shape[0]), int(Y.shape[1])
        assert tuple(X.shape) == tuple(V.shape) == (N, nsig), "Y, X and V has to have the same number of samples"
        assert all(a.stride(0) == 1 and a.stride(1) == N for a in (Y, X, V)), "device inputs must be column-major (N x nsig, e.g. A.T.contiguous().T)"
    else:
        Yh, Xh, Vh = (np.asfortranarray(_host(a), dtype=np.float64) for a in (Y, X, V))
        N, nsig = Yh.shape
        assert Xh.shape == Vh.shape == (N, nsig), "Y, X and V has to have the same number of samples"
    Nf, Nv = len(w), int(Nv)
    g = SlicedSeparableSum.frequency_groups(λ, Nf, 2 * Nv) if proxg is None else proxg
    kind, param, glen = g.device_params(2 * Nf * Nv)
    dv = None if devices is None else np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
    if dv is not None:
        ngpus = len(dv)
    m = Nf * Nv
    re, im = np.zeros((m, nsig), order="F"), np.zeros((m, nsig), order="F")
    its = np.zeros(nsig, dtype=np.int64)
    ptr = (lambda a: C.c_void_p(a.data_ptr())) if dev_in else out_ptr
    if dev_in:
        import torch
        torch.cuda.current_stream(Y.device).synchronize()             # the library works on its own streams
    check(lib().lpvs_lpv_signals_multi_f64(ptr(Yh), ptr(Xh), ptr(Vh), N, nsig, out_ptr(w), Nf, Nv, int(bool(normalize)), int(kind), float(param),
                                           int(glen), float(μ), float(tol), int(iters), None if dv is None else out_ptr(dv), int(ngpus), int(in_flight),
                                           out_ptr(re), out_ptr(im), out_ptr(its)))
    return re + 1j * im, its


def ls_spectral_lpv(Y, X, V, w, Nv, λ=1e-8, coulomb=False, normalize=True, device=0, covariance=True):
    """``ls_spectral_lpv(Y,X,V,w,Nv; λ, coulomb, normalize)`` (src/lsfft.jl:239-259) -> :class:`SpectralExt`.

    Ridge solve ``[Ar; λI] \\ [Y; 0]`` in normal-equation form on the device Gram (built in the permuted column
    order; ridge and solution are permutation-invariant and are un-permuted by the same packing as the sparse path).
    The residual statistics come from the same Gram, with the constant signal as a second right-hand side:
    ``‖e‖² = x'Gx − 2b'x + Y'Y``, ``Σe = (Φ'1)'x − ΣY`` ⇒ ``var(e)``; ``Σ = var(e)·(AA'AA + λI)⁻¹`` (:252-254, λ not
    squared, as written) in the reference's ``[re; im]`` parameter order; the fva warning of :255-256 is issued."""
    w = _host_vec(w) if not _lib.is_device_array(w) else w
    Nv = int(Nv)
    Yh = _host(Y)
    def ridge(prob):
        try:
            return prob.solve_ridge(λ * λ)
        except _lib.NumericError as e:
            # (G + λ²I) is singular to working precision (e.g. more unknowns than samples with the default λ = 1e-8): the
            # normal equations cannot reproduce the reference there, its QR of [Ar; λI] can.  Same route, host LAPACK, on
            # the regressor the device kernel materialises (src/utilities.jl:49-54).
            log.info("ls_spectral_lpv: %s; solving [A; λI] \\ [Y; 0] by QR on the host", e)
            Phi = lpv_regressor(X, V, w, Nv, normalize, coulomb, permuted=True)
            return _host_qr_ridge(Phi, Yh, λ)

    if not covariance:
        with Problem.lpv(Y, X, V, w, Nv, normalize, coulomb, device=device) as prob:
            params = prob.pack(ridge(prob))
        return SpectralExt(Y, X, V, w, Nv, λ, coulomb, normalize, params, None)
    Y2 = np.stack([Yh, np.ones_like(Yh)], axis=1)
    with Problem.lpv_multi(Y2, X, V, w, Nv, normalize, coulomb, device=device) as prob:
        x = ridge(prob)                                  # first right-hand side = Y
        params = prob.pack(x)
        G, _ = prob.get_gram()
        B = prob.get_rhs()
        try:
            Minv = prob.get_inverse_refined(λ)               # Σ is this inverse itself: refined, as the solves are
        except _lib.NumericError:
            Minv = np.linalg.inv(G + λ * np.eye(G.shape[0]))   # inv(AA'AA + λI) as the reference evaluates it (:253)
        Nf, nb = prob.Nf, prob.nb
    N = len(Yh)
    e2 = float(x @ (G @ x) - 2.0 * (B[:, 0] @ x) + Yh @ Yh)         # ‖AA·x − Y‖²
    esum = float(B[:, 1] @ x - Yh.sum())
    var_e = (e2 - esum * esum / N) / (N - 1)                         # var(e), corrected (Statistics.var)
    var_y = float(np.var(Yh, ddof=1))
    # un-permute: reference order u = c·Nf·nb + j·Nf + f  <-  device order p = f·2nb + c·nb + j
    f_, c_, j_ = np.meshgrid(np.arange(Nf), np.arange(2), np.arange(nb), indexing="ij")
    perm = np.empty(2 * Nf * nb, dtype=np.int64)
    perm[(c_ * Nf * nb + j_ * Nf + f_).ravel()] = (f_ * 2 * nb + c_ * nb + j_).ravel()
    Sigma = var_e * Minv[np.ix_(perm, perm)]
    fva = 1.0 - var_e / var_y                                        # :255
    if fva < 0.9:
        import warnings
        warnings.warn(f"Fraction of variance explained = {fva}")    # :256
    return SpectralExt(Y, X, V, w, Nv, λ, coulomb, normalize, params, Sigma)


def windowpsd_sparse_batched(y, t, freqs, n, noverlap=-1, W=None, proxg=None, λ=1.0, μ=0.05, tol=1e-5, iters=10000,
                             win_lo=0, win_hi=None, device=0, as_written=True):
    """All windows ``[win_lo, win_hi)`` of ``Windows2(y,t,n,noverlap)`` solved together on one GPU with the weighted
    ``ls_sparse_spectral(y,t,f,W)`` estimator (src/lasso.jl:105-126): one batch of panels / Gram matrices /
    factorisations / ADMM iterations per launch.  Returns ``(x [nwin x Nf complex], S_partial [Nf], iters [nwin])``
    where ``S_partial = Σ_i |x_i|²`` in window order (not yet divided by k²)."""
    ky, py, Ly = as_f64(y)
    kt, pt, Lt = as_f64(t)
    kf, pf, Nf = as_f64(freqs)
    kw, pw, nW = as_f64(W)
    assert Ly == Lt, "y and t has to be the same length"
    assert W is None or nW == n, "W must have one weight per window sample"
    k = C.c_int64(0)
    check(lib().lpvs_window_count(Ly, int(n), int(noverlap), C.byref(k)))
    win_hi = int(k.value) if win_hi is None else int(win_hi)
    nwin = win_hi - int(win_lo)
    proxg = NormL1(λ) if proxg is None else proxg
    kind, param, glen = proxg.device_params(2 * Nf)
    xre, xim = np.zeros((max(nwin, 1), Nf)), np.zeros((max(nwin, 1), Nf))
    S, its = np.zeros(Nf), np.zeros(max(nwin, 1), dtype=np.int64)
    sign = _lib.LINEAR_QUADRATIC_AS_WRITTEN if as_written else _lib.LINEAR_LEAST_SQUARES
    check(lib().lpvs_windowpsd_sparse_f64(py, pt, Ly, int(n), int(noverlap), pw, pf, Nf, int(kind), float(param), int(glen),
                                          float(μ), float(tol), int(iters), int(sign), int(win_lo), win_hi, int(device),
                                          out_ptr(xre), out_ptr(xim), out_ptr(S), out_ptr(its)))
    return (xre + 1j * xim)[:nwin], S, its[:nwin]


def windowpsd_last_timing():
    """Phase times (HIP events) of this thread's last batched-window call."""
    o = np.zeros(12)
    check(lib().lpvs_windowpsd_last_timing(out_ptr(o), 12))
    d = dict(gram_rhs_ms=o[0], inverse_ms=o[1], solve_ms=o[2], windows=int(o[3]), passes=int(o[6]), structured_gram=bool(o[7]),
             gram_form=("dense", "ap", "ap-nufft")[int(o[7])], one_launch_iteration=bool(o[9]), reads_32_bits=int(o[9]) == 2,
             rccl_gather_ranks=int(o[10]), multi_devices=int(o[11]))
    if o[4] > 0:
        d["matvec_us_per_iteration"] = float(o[4]); d["matvec_windows"] = int(o[5]); d["matvec_bytes_per_launch"] = float(o[8])

    return d


def _engine_args(estimator, kwargs, nreg):
    """Map the reference's estimator + kwargs onto the engine's arguments, or None when that combination has no batched
    form (user-supplied estimator, per-iteration callback, unknown keywords -> the reference's sequential loop)."""
    kw = dict(kwargs)
    kw.pop("device", None)
    if estimator is ls_spectral:                                       # 4-argument weighted method, src/lsfft.jl:74-80
        if kw.pop("verbose", False) or set(kw) - {"λ"}:
            return None
        return dict(estimator=_lib.EST_DENSE, lam=float(kw.get("λ", 1e-10)), prox=(_lib.PROX_L1, 0.0, 0), μ=0.05, tol=0.0, iters=0,
                    sign=_lib.LINEAR_LEAST_SQUARES)
    if estimator is ls_sparse_spectral:                                # 4-argument weighted method, src/lasso.jl:105-126
        if kw.get("cb") is not None or set(kw) - {"λ", "proxg", "μ", "tol", "iters", "printerval", "cb", "init", "out"}:
            return None                                                # a per-iteration callback needs the host loop
        pg = kw.get("proxg")
        pg = NormL1(kw.get("λ", 1.0)) if pg is None else pg
        if not hasattr(pg, "device_params"):
            return None
        μ = kw.get("μ", 0.05)
        assert 0 <= μ <= 1, "μ should be ≤ 1"                          # src/lasso.jl:143
        init = bool(kw.get("init", False))                             # x0 = fourier_solve(A, y, zerofreq, λ): one batched ridge solve (:112)
        return dict(estimator=_lib.EST_SPARSE_INIT if init else _lib.EST_SPARSE, lam=float(kw.get("λ", 1.0)) if init else 0.0,
                    prox=pg.device_params(nreg), μ=float(μ), tol=float(kw.get("tol", 1e-5)),
                    iters=int(kw.get("iters", 10000)), sign=_lib.LINEAR_QUADRATIC_AS_WRITTEN)
    return None


def windows_estimate(Y, t, freqs, n, noverlap, W, eng, win_lo=0, win_hi=None, device=0):
    """The batched-window engine (``lpvs_windows_estimate_f64``): ``Y`` is a list of signals sharing ``t``; returns
    ``x[ns][nwin][Nf]`` complex and the iteration counts ``[ns][nwin]``."""
    # Float32 entry points only when y, t and freqs are ALL Float32: the window drivers call the 4-argument estimator, whose regressor
    # is evaluated in the eltype of t and freqs (src/lsfft.jl:121 -> src/lasso.jl:111); Float32 y with Float64 t stays exact in t
    if all(is_f32(y) and not _lib.is_device_array(y) for y in Y) and _all_f32(t, freqs):      # lpvs_windows_estimate_f32
        keep = np.ascontiguousarray(np.stack([np.asarray(y, dtype=np.float32) for y in Y]))
        ns, Ly = keep.shape
        th = np.ascontiguousarray(np.asarray(_host(t), dtype=np.float32)); fh = np.ascontiguousarray(np.asarray(_host(freqs), dtype=np.float32))
        Wh = None if W is None else np.ascontiguousarray(np.asarray(_host(W), dtype=np.float32))
        assert Ly == len(th), "y and t has to be the same length"
        assert Wh is None or len(Wh) == n, "W must have one weight per window sample"
        k = C.c_int64(0)
        check(lib().lpvs_window_count(Ly, int(n), int(noverlap), C.byref(k)))
        win_hi = int(k.value) if win_hi is None else int(win_hi)
        nwin, Nf = win_hi - int(win_lo), len(fh)
        xre, xim = np.zeros((ns, max(nwin, 1), Nf), dtype=np.float32), np.zeros((ns, max(nwin, 1), Nf), dtype=np.float32)
        its = np.zeros((ns, max(nwin, 1)), dtype=np.int64)
        kind, param, glen = eng["prox"]
        check(lib().lpvs_windows_estimate_f32(out_ptr(keep), ns, out_ptr(th), Ly, int(n), int(noverlap), None if Wh is None else out_ptr(Wh), out_ptr(fh), Nf,
                                              int(eng["estimator"]), float(eng["lam"]), int(kind), float(param), int(glen), float(eng["μ"]), float(eng["tol"]),
                                              int(eng["iters"]), int(eng["sign"]), int(win_lo), win_hi, int(device), out_ptr(xre), out_ptr(xim), out_ptr(its)))
        return (xre + 1j * xim).astype(np.complex64)[:, :nwin], its[:, :nwin]
    Ys = [as_f64(y) for y in Y]
    ns, Ly = len(Ys), Ys[0][2]
    assert all(e[2] == Ly for e in Ys), "signals must have the same length"
    kt, pt, Lt = as_f64(t)
    kf, pf, Nf = as_f64(freqs)
    kw, pw, nW = as_f64(W)
    assert Ly == Lt, "y and t has to be the same length"
    assert W is None or nW == n, "W must have one weight per window sample"
    k = C.c_int64(0)
    check(lib().lpvs_window_count(Ly, int(n), int(noverlap), C.byref(k)))
    win_hi = int(k.value) if win_hi is None else int(win_hi)
    nwin = win_hi - int(win_lo)
    dev_in = all(_lib.is_device_array(y) for y in Y)
    if ns == 1:
        keep, pY = Ys[0][0], Ys[0][1]
    elif dev_in:
        import torch
        keep = torch.stack([y.reshape(-1) for y in Y]).contiguous()   # [ns][L] row-major == L x ns column-major
        pY = C.c_void_p(keep.data_ptr())
    else:
        keep = np.ascontiguousarray(np.stack([_host(y) for y in Y]))
        pY = out_ptr(keep)
    xre, xim = np.zeros((ns, max(nwin, 1), Nf)), np.zeros((ns, max(nwin, 1), Nf))
    its = np.zeros((ns, max(nwin, 1)), dtype=np.int64)
    kind, param, glen = eng["prox"]
    check(lib().lpvs_windows_estimate_f64(pY, ns, pt, Ly, int(n), int(noverlap), pw, pf, Nf, int(eng["estimator"]), float(eng["lam"]),
                                          int(kind), float(param), int(glen), float(eng["μ"]), float(eng["tol"]), int(eng["iters"]),
                                          int(eng["sign"]), int(win_lo), win_hi, int(device), out_ptr(xre), out_ptr(xim), out_ptr(its)))
    return (xre + 1j * xim)[:, :nwin], its[:, :nwin]


def windows_estimate_state(Y, t, freqs, n, noverlap, W, eng, win_lo=0, win_hi=None, device=0):
    """``lpvs_windows_estimate_state_f64``: the engine of :func:`windows_estimate`, returning the raw ADMM state ``x, z, u`` of every
    problem (each ``[ns][nwin][Nreg]`` in the reference's ordering ``[re; im]``: the ``(x, z)`` of src/lasso.jl:170 and the dual variable) and
    the iteration counts ``[ns][nwin]``.  Sparse estimators, Float64."""
    Ys = [as_f64(y) for y in Y]
    ns, Ly = len(Ys), Ys[0][2]
    assert all(e[2] == Ly for e in Ys), "signals must have the same length"
    kt, pt, Lt = as_f64(t)
    kf, pf, Nf = as_f64(freqs)
    kw, pw, nW = as_f64(W)
    assert Ly == Lt, "y and t has to be the same length"
    assert W is None or nW == n, "W must have one weight per window sample"
    k = C.c_int64(0)
    check(lib().lpvs_window_count(Ly, int(n), int(noverlap), C.byref(k)))
    win_hi = int(k.value) if win_hi is None else int(win_hi)
    nwin = win_hi - int(win_lo)
    if ns == 1:
        keep, pY = Ys[0][0], Ys[0][1]
    elif all(_lib.is_device_array(y) for y in Y):
        import torch
        keep = torch.stack([y.reshape(-1) for y in Y]).contiguous()
        pY = C.c_void_p(keep.data_ptr())
    else:
        keep = np.ascontiguousarray(np.stack([_host(y) for y in Y]))
        pY = out_ptr(keep)
    zf = C.c_int64(0)
    fh = np.ascontiguousarray(np.asarray(_host(freqs), dtype=np.float64))
    check(lib().lpvs_check_freq_f64(out_ptr(fh), Nf, C.byref(zf)))
    nreg = 2 * Nf - 1 if zf.value else 2 * Nf
    x, z, u = (np.zeros((ns, max(nwin, 1), nreg)) for _ in range(3))
    its = np.zeros((ns, max(nwin, 1)), dtype=np.int64)
    kind, param, glen = eng["prox"]
    check(lib().lpvs_windows_estimate_state_f64(pY, ns, pt, Ly, int(n), int(noverlap), pw, pf, Nf, int(eng["estimator"]), float(eng["lam"]),
                                                int(kind), float(param), int(glen), float(eng["μ"]), float(eng["tol"]), int(eng["iters"]),
                                                int(eng["sign"]), int(win_lo), win_hi, int(device), out_ptr(x), out_ptr(z), out_ptr(u), out_ptr(its)))
    return x[:, :nwin], z[:, :nwin], u[:, :nwin], its[:, :nwin]


def windows_estimate_multi(Y, t, freqs, n, noverlap, W, eng, ngpus=0, devices=None):
    """``lpvs_windows_estimate_multi_f64``: ALL windows, split into contiguous ranges over ``ngpus`` devices driven by
    this one process (a host thread per device), the coefficients gathered by one RCCL all-gather.  Same return value as
    :func:`windows_estimate` over the full window range."""
    f32 = all(is_f32(y) and not _lib.is_device_array(y) for y in Y) and _all_f32(t, freqs)      # all-Float32 call: lpvs_windows_estimate_multi_f32
    dt = np.float32 if f32 else np.float64
    Ys = [np.ascontiguousarray(np.asarray(_host(y), dtype=dt)) for y in Y]
    ns, Ly = len(Ys), len(Ys[0])
    assert all(len(e) == Ly for e in Ys), "signals must have the same length"
    keep = np.ascontiguousarray(np.stack(Ys))
    th = np.ascontiguousarray(np.asarray(_host(t), dtype=dt)); fh = np.ascontiguousarray(np.asarray(_host(freqs), dtype=dt))
    Wh = None if W is None else np.ascontiguousarray(np.asarray(_host(W), dtype=dt))
    assert Ly == len(th), "y and t has to be the same length"
    assert Wh is None or len(Wh) == n, "W must have one weight per window sample"
    k = C.c_int64(0)
    check(lib().lpvs_window_count(Ly, int(n), int(noverlap), C.byref(k)))
    k, Nf = int(k.value), len(fh)
    dv = None if devices is None else np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
    if dv is not None:
        ngpus = len(dv)
    xre, xim = np.zeros((ns, max(k, 1), Nf), dtype=dt), np.zeros((ns, max(k, 1), Nf), dtype=dt)
    its = np.zeros((ns, max(k, 1)), dtype=np.int64)
    kind, param, glen = eng["prox"]
    check((lib().lpvs_windows_estimate_multi_f32 if f32 else lib().lpvs_windows_estimate_multi_f64)(out_ptr(keep), ns, out_ptr(th), Ly, int(n), int(noverlap), None if Wh is None else out_ptr(Wh),
                                                out_ptr(fh), Nf, int(eng["estimator"]), float(eng["lam"]), int(kind), float(param), int(glen),
                                                float(eng["μ"]), float(eng["tol"]), int(eng["iters"]), int(eng["sign"]),
                                                None if dv is None else out_ptr(dv), int(ngpus), out_ptr(xre), out_ptr(xim), out_ptr(its)))
    return (xre + 1j * xim)[:, :k], its[:, :k]


def windowcsd_batched(y, u, t, freqs, n, noverlap, W, eng, win_lo=0, win_hi=None, device=0):
    """``lpvs_windowcsd_f64``: the accumulators ``(Syu, Syy, Suu)`` over the windows ``[win_lo, win_hi)`` in window order
    (one Gram / factorisation per window, two right-hand sides), plus the per-window ``xy, xu``."""
    f32 = (is_f32(y) and is_f32(u) and not _lib.is_device_array(y) and not _lib.is_device_array(u)
           and _all_f32(t, freqs))                             # all-Float32 call: lpvs_windowcsd_f32 (see windows_estimate)
    dt = np.float32 if f32 else np.float64
    conv = (lambda a: as_f32(None if a is None else np.asarray(_host(a), dtype=np.float32))) if f32 else as_f64
    ky, py, Ly = conv(y)
    ku, pu, Lu = conv(u)
    kt, pt, Lt = conv(t)
    kf, pf, Nf = conv(freqs)
    kw, pw, nW = conv(W)
    assert Ly == Lu == Lt, "y, u and t has to be the same length"
    assert W is None or nW == n, "W must have one weight per window sample"
    k = C.c_int64(0)
    check(lib().lpvs_window_count(Ly, int(n), int(noverlap), C.byref(k)))
    win_hi = int(k.value) if win_hi is None else int(win_hi)
    nwin = win_hi - int(win_lo)
    sre, sim, syy, suu = (np.zeros(Nf, dtype=dt) for _ in range(4))
    xre, xim = np.zeros((2, max(nwin, 1), Nf), dtype=dt), np.zeros((2, max(nwin, 1), Nf), dtype=dt)
    kind, param, glen = eng["prox"]
    check((lib().lpvs_windowcsd_f32 if f32 else lib().lpvs_windowcsd_f64)(py, pu, pt, Ly, int(n), int(noverlap), pw, pf, Nf, int(eng["estimator"]), float(eng["lam"]), int(kind),
                                   float(param), int(glen), float(eng["μ"]), float(eng["tol"]), int(eng["iters"]), int(eng["sign"]),
                                   int(win_lo), win_hi, int(device), out_ptr(sre), out_ptr(sim), out_ptr(syy), out_ptr(suu), out_ptr(xre),
                                   out_ptr(xim), None))
    x = (xre + 1j * xim)[:, :nwin]
    return sre + 1j * sim, syy, suu, x[0], x[1]


@_with_options
def ls_windowpsd(y, t, freqs=None, nw=8, noverlap=-1, window_func=rect, estimator=None, batched=True, **kwargs):
    """``ls_windowpsd(y,t,freqs; nw, noverlap, window_func, estimator=ls_spectral, kwargs...)``
    (src/lsfft.jl:112-126) -> ``(S, freqs)``.  ``estimator`` is any callable ``(y,t,f,W; kw...) -> (x, f)``
    (plugin boundary #1); it is always called with the window vector, as in the reference (:121).

    With this package's ``ls_spectral`` / ``ls_sparse_spectral`` as the estimator (and no per-iteration callback) the windows
    are solved as ONE device batch (per-iteration progress lines are not printed); ``batched=False`` forces the reference's
    sequential loop."""
    estimator = ls_spectral if estimator is None else estimator
    n = len(y) // nw                                                # :113
    if freqs is None:
        freqs = default_freqs(t, n=n)                               # :114
    windows = Windows2(y, t, n, noverlap, window_func)              # :115
    k = len(windows)                                                # :116
    ngpus = kwargs.pop("ngpus", 1)                                  # extension: devices driven by this process (0 = all visible)
    eng = _engine_args(estimator, kwargs, 2 * len(freqs)) if (batched and k > 0) else None
    if eng is not None:
        if ngpus != 1:
            x, _ = windows_estimate_multi([y], t, freqs, n, windows.noverlap, windows.W, eng, ngpus=ngpus)
        else:
            x, _ = windows_estimate([y], t, freqs, n, windows.noverlap, windows.W, eng, device=kwargs.get("device", 0))
        S = np.zeros(len(freqs))
        for i in range(k):
            S += abs2(x[0, i])                                      # :122, window order
        return S / k ** 2, freqs                                    # :125
    S = np.zeros(len(freqs))
    for yi, ti in windows:                                          # :120
        x = estimator(yi, ti, freqs, windows.W, **kwargs)[0]        # :121
        S += abs2(x)                                                # :122
    return S / k ** 2, freqs                                        # :125


@_with_options
def ls_windowcsd(y, u, t, freqs=None, nw=10, noverlap=-1, window_func=rect, estimator=None, batched=True, **kwargs):
    """``ls_windowcsd(y,u,t,freqs; nw, noverlap, window_func, estimator=ls_spectral)`` (src/lsfft.jl:140-156):
    cross spectral density, ``S += xy .* conj(xu)`` over the windows, returned as ``S/nw`` (the recomputed window count).

    Batched on the device engine as :func:`ls_windowpsd` is: one Gram and one factorisation per window serve both signals."""
    estimator = ls_spectral if estimator is None else estimator
    n = len(y) // nw
    if freqs is None:
        freqs = default_freqs(t, n=n)
    wy = Windows2(y, t, n, noverlap, window_func)
    wu = Windows2(u, t, n, noverlap, window_func)
    k = len(wy)
    ngpus = kwargs.pop("ngpus", 1)
    eng = _engine_args(estimator, kwargs, 2 * len(freqs)) if (batched and k > 0) else None
    if eng is not None and ngpus != 1:
        x, _ = windows_estimate_multi([y, u], t, freqs, n, wy.noverlap, wy.W, eng, ngpus=ngpus)
        S = np.zeros(len(freqs), dtype=np.complex128)
        for i in range(k):
            S = S + _mul_conj(x[0, i], x[1, i])                     # :152, window order
        return S / k, freqs
    if eng is not None:
        Syu, _, _, _, _ = windowcsd_batched(y, u, t, freqs, n, wy.noverlap, wy.W, eng, device=kwargs.get("device", 0))
        return Syu / k, freqs
    S = np.zeros(len(freqs), dtype=np.complex128)
    for (yi, ti), (ui, _) in zip(wy, wu):
        xy = estimator(yi, ti, freqs, wy.W, **kwargs)[0]
        xu = estimator(ui, ti, freqs, wu.W, **kwargs)[0]
        S = S + _mul_conj(xy, xu)                                 # src/lsfft.jl:152
    return S / k, freqs


@_with_options
def ls_cohere(y, u, t, freqs=None, nw=10, noverlap=-1, estimator=None, batched=True, **kwargs):
    """``ls_cohere(y,u,t,freqs; nw, noverlap, estimator=ls_spectral)`` (src/lsfft.jl:176-193): magnitude-squared
    coherence over Hann-weighted windows (``Windows3(y,t,u,n,noverlap,hanning)``, :182)."""
    from .windows import hanning
    estimator = ls_spectral if estimator is None else estimator
    n = len(y) // nw
    if freqs is None:
        freqs = default_freqs(t, n=n)
    windows = Windows3(y, t, u, n, noverlap, hanning)
    ngpus = kwargs.pop("ngpus", 1)
    eng = _engine_args(estimator, kwargs, 2 * len(freqs)) if (batched and len(windows) > 0) else None
    if eng is not None and ngpus != 1:
        x, _ = windows_estimate_multi([y, u], t, freqs, n, windows.noverlap, windows.W, eng, ngpus=ngpus)
        Syy, Suu = np.zeros(len(freqs)), np.zeros(len(freqs))
        Syu = np.zeros(len(freqs), dtype=np.complex128)
        for i in range(x.shape[1]):                                 # :183-190, window order
            Syu += _mul_conj(x[0, i], x[1, i]); Syy += abs2(x[0, i]); Suu += abs2(x[1, i])
        with np.errstate(invalid="ignore", divide="ignore"):        # 0/0 where neither signal has the frequency: NaN, silently, as in Julia
            return abs2(Syu) / (Suu * Syy), freqs
    if eng is not None:
        Syu, Syy, Suu, _, _ = windowcsd_batched(y, u, t, freqs, n, windows.noverlap, windows.W, eng, device=kwargs.get("device", 0))
        with np.errstate(invalid="ignore", divide="ignore"):
            return abs2(Syu) / (Suu * Syy), freqs                   # :191
    Syy, Suu = np.zeros(len(freqs)), np.zeros(len(freqs))
    Syu = np.zeros(len(freqs), dtype=np.complex128)
    for yi, ti, ui in windows:
        xy = np.asarray(estimator(yi, ti, freqs, windows.W, **kwargs)[0])
        xu = np.asarray(estimator(ui, ti, freqs, windows.W, **kwargs)[0])
        Syu += _mul_conj(xy, xu)
        Syy += abs2(xy)
        Suu += abs2(xu)
    with np.errstate(invalid="ignore", divide="ignore"):
        return abs2(Syu) / (Suu * Syy), freqs


@_with_options
def ls_windowpsd_lpv(Y, X, V, w, Nv, nw=10, noverlap=0, in_flight=4, **kwargs):
    """src/lsfft.jl:267-277.  The windows' regressors share nothing (each has its own samples of X and V): their Grams are built
    ``in_flight`` at a time (an extension; 1 = one after the other) into one batch, whose factorisations and refined ridge solves
    then run for all windows at once (``lpvs_windowpsd_lpv_f64``; 40 windows of 5000 samples with 1024 unknowns each: 19 ms with four
    Gram builds in flight, 22 with two, 35 with one -- the per-window loop of single-handle solves: 129 ms).  The sum over windows is taken in window order (:274), so the
    result does not depend on ``in_flight``; windows explaining less than 0.9 of their variance warn as the reference does (:255-256)."""
    w = np.ravel(_host(w))
    S = np.zeros(len(w))
    # the library's own driver (lpvs_windowpsd_lpv_f64: the same device solves, the library's worker threads) whenever the call has only
    # what it takes; a singular window (LPVS_ENUMERIC) sends the whole call down the per-window path below, which has the host-QR route
    if set(kwargs) <= {"λ", "coulomb", "normalize", "device"} and not any(_lib.is_device_array(a) for a in (Y, X, V)) and not _all_f32(Y, X, V):
        Yh, Xh, Vh = (np.ascontiguousarray(_host(a), dtype=np.float64) for a in (Y, X, V))
        assert len(Yh) == len(Xh) == len(Vh), "y, t and v has to be the same length"   # src/windows.jl:96
        wv = np.ascontiguousarray(w, dtype=np.float64)
        kcnt = C.c_int64(0)
        check(lib().lpvs_window_count(len(Yh), len(Yh) // int(nw), int(noverlap), C.byref(kcnt)))
        fva = np.ones(max(int(kcnt.value), 1))
        try:
            check(lib().lpvs_windowpsd_lpv_f64(out_ptr(Yh), out_ptr(Xh), out_ptr(Vh), len(Yh), out_ptr(wv), len(wv), int(Nv), len(Yh) // int(nw), int(noverlap),
                                               float(kwargs.get("λ", 1e-8)), int(bool(kwargs.get("normalize", True))), int(bool(kwargs.get("coulomb", False))),
                                               int(kwargs.get("device", 0)), max(1, min(8, int(in_flight))), out_ptr(S), out_ptr(fva)))
            for v in fva[:int(kcnt.value)]:
                if v < 0.9:                                            # src/lsfft.jl:255-256, once per window as the reference's loop does
                    import warnings
                    warnings.warn(f"Fraction of variance explained = {v}")
            return S
        except _lib.NumericError as e:
            log.info("ls_windowpsd_lpv: %s; per-window path", e)
            S = np.zeros(len(w))
    windows = list(Windows3(Y, X, V, len(Y) // nw, noverlap, rect))
    kwargs.setdefault("covariance", False)                         # the driver reads the parameters only (:273-274): no Σ, no second inverse
    solve = lambda win: ls_spectral_lpv(win[0], win[1], win[2], w, Nv, **kwargs)
    if in_flight > 1 and len(windows) > 1:
        from concurrent.futures import ThreadPoolExecutor
        opts = {k: get_default_option(k) for k in _lib.OPTIONS}    # (the option defaults are thread-local: carried into the workers)
        def worker(win):
            with default_options(**opts):
                return solve(win)
        with ThreadPoolExecutor(max_workers=int(in_flight)) as pool:
            ses = list(pool.map(worker, windows))                  # (ctypes releases the GIL inside the library; results in window order)
    else:
        ses = [solve(win) for win in windows]
    for se in ses:
        rp = reshape_params(se.x, len(w))
        S = S + abs2(rp.sum(axis=1))
    return S


# --------------------------------------------------------------------------- autocov / autocor at arbitrary sample times (src/autocov.jl)
_EXACT_INT = 2 ** 52   # integer times are carried as float64: |t| < 2^52 keeps t and every difference exact


def _is_torch(a):
    return hasattr(a, "data_ptr") and hasattr(a, "dtype") and hasattr(a, "is_cuda")


def _time_kind(t):
    """'int' (a range or integer times: tau is int64), 'f32' or 'f64'."""
    if isinstance(t, range):
        return "int"
    if _is_torch(t):
        import torch
        return "f32" if t.dtype == torch.float32 else ("f64" if t.dtype.is_floating_point else "int")
    a = np.asarray(t)
    return "f32" if a.dtype == np.float32 else ("int" if a.dtype.kind in "iub" else "f64")


def _value_kind(y):
    if _is_torch(y):
        import torch
        return "f32" if y.dtype == torch.float32 else "f64"
    return "f32" if np.asarray(y).dtype == np.float32 else "f64"


def _is_segmented(y):
    """The vector-of-vectors form (src/autocov.jl:1-16): a list / tuple of signals."""
    return isinstance(y, (list, tuple)) and len(y) > 0 and (isinstance(y[0], (list, tuple, range, np.ndarray)) or _is_torch(y[0]))


def isequidistant(t):
    """src/autocov.jl:112-121.  A ``range`` is equidistant iff its step is positive; a vector iff ``d = t[1]-t[0] > 0`` and
    ``abs(abs(t[i]-t[i-1]) - d) < 20d*eps()`` for every i (eps of Float64).  Fewer than 2 samples: ValueError."""
    if isinstance(t, range):
        return t.step > 0
    out = C.c_int32(0)
    if _time_kind(t) == "f32":
        kt, pt, N = as_f32(t)
        check(lib().lpvs_isequidistant_f32(pt, N, C.byref(out)))
    else:
        kt, pt, N = as_f64(t)
        check(lib().lpvs_isequidistant_f64(pt, N, C.byref(out)))
    return bool(out.value)


def _segment_vec(a, kind, dev):
    """One segment as a contiguous 1-D array of the computing eltype (float32 / float64), on the device when dev is set."""
    if isinstance(a, range):
        a = np.arange(a.start, a.stop, a.step, dtype=np.int64)
    if _is_torch(a):
        import torch
        v = a.reshape(-1).to(torch.float32 if kind == "f32" else torch.float64)
        return v.to(f"cuda:{dev}") if dev is not None else v.cpu().numpy()
    v = np.ravel(np.asarray(a)).astype(np.float32 if kind == "f32" else np.float64)
    if dev is not None:
        import torch
        return torch.from_numpy(np.ascontiguousarray(v)).to(f"cuda:{dev}")
    return np.ascontiguousarray(v)


def _autofun(kind, t, y, maxlag, normalize, device):
    segmented = _is_segmented(y)
    ts, ys = (list(t), list(y)) if segmented else ([t], [y])
    if len(ts) != len(ys):
        raise ValueError(f"t has {len(ts)} segments, y has {len(ys)}")
    for a, b in zip(ts, ys):
        if len(a) != len(b):
            raise ValueError("t and y must be the same length")        # src/autocov.jl:40
    tk = {_time_kind(a) for a in ts}
    yk = {_value_kind(b) for b in ys}
    t_kind = "int" if tk == {"int"} else ("f32" if tk == {"f32"} else "f64")   # vcat's promotion of the segments' tau
    y_kind = "f32" if yk == {"f32"} else "f64"
    if t_kind == "f32" and y_kind != "f32":
        raise TypeError("float32 times with float64 values: pass both as float32 or both as float64")
    if t_kind == "int":
        for a in ts:
            if len(a) and max(abs(int(min(a))), abs(int(max(a)))) >= _EXACT_INT:
                raise ValueError("integer sample times must satisfy |t| < 2^52")
    ckind = "f32" if t_kind == "f32" else "f64"
    on_dev = any(_is_torch(a) and a.is_cuda for a in ts + ys)
    dev = next(a.device.index for a in ts + ys if _is_torch(a) and a.is_cuda) if on_dev else None
    lens = [len(a) for a in ts]
    seg_off = np.zeros(len(lens) + 1, dtype=np.int64)
    seg_off[1:] = np.cumsum(lens)
    tv = [_segment_vec(a, ckind, dev) for a in ts]
    yv = [_segment_vec(b, ckind, dev) for b in ys]
    if on_dev:
        import torch
        tc, yc = torch.cat(tv), torch.cat(yv)
        torch.cuda.current_stream(tc.device).synchronize()
        pt, py = C.c_void_p(tc.data_ptr()), C.c_void_p(yc.data_ptr())
        device = dev
    else:
        tc, yc = np.concatenate(tv), np.concatenate(yv)
        pt, py = out_ptr(tc), out_ptr(yc)
    fn = lib().lpvs_autofun_f32 if ckind == "f32" else lib().lpvs_autofun_f64
    n = C.c_int64(0)
    ml = float(maxlag)
    args = (kind, pt, py, out_ptr(seg_off), len(lens), ml, int(bool(normalize)), int(device))
    check(fn(*args, None, None, 0, C.byref(n)))                        # count only
    P = int(n.value)
    if on_dev:
        import torch
        dt = torch.float32 if ckind == "f32" else torch.float64
        tau, acf = torch.empty(P, dtype=dt, device=tc.device), torch.empty(P, dtype=dt, device=tc.device)
        check(fn(*args, C.c_void_p(tau.data_ptr()), C.c_void_p(acf.data_ptr()), P, C.byref(n)))
        if t_kind == "int":
            tau = tau.to(torch.int64)
        if y_kind == "f32":
            acf = acf.to(torch.float32)
        return tau, acf
    dt = np.float32 if ckind == "f32" else np.float64
    tau, acf = np.empty(P, dtype=dt), np.empty(P, dtype=dt)
    check(fn(*args, out_ptr(tau), out_ptr(acf), P, C.byref(n)))
    if t_kind == "int":
        tau = tau.astype(np.int64)
    if y_kind == "f32":
        acf = acf.astype(np.float32)
    return tau, acf


def autocov(t, y, maxlag, normalize=False, device=0):
    """src/autocov.jl:35-56, :125-147 -> ``(τ, acf)``: the autocovariance of ``y`` sampled at times ``t`` over every sample pair
    with ``|t[i+j]-t[i]| <= maxlag``, sorted by τ (stable).  ``t`` / ``y`` may be arrays, ``range``s (t), or lists of segments (the
    vector-of-vectors form, src/autocov.jl:1-16).  τ has the eltype of ``t`` (int64 for integer times), acf that of ``y``.  Device
    (torch CUDA) inputs give device tensors; host inputs give numpy arrays."""
    return _autofun(_lib.ACF_COV, t, y, maxlag, normalize, device)


def autocor(t, y, maxlag, normalize=False, device=0):
    """src/autocov.jl:78-100, :149-176: as :func:`autocov`, normalised (by dot(y,y) on the equidistant branch, by var(y) otherwise)."""
    return _autofun(_lib.ACF_COR, t, y, maxlag, normalize, device)


def autofun_last_timing():
    """HIP-event phase times (ms) of this thread's last autocov / autocor call (the last of its two library calls: the one that wrote
    the outputs)."""
    o = np.zeros(8)
    check(lib().lpvs_autofun_last_timing(out_ptr(o), 8))
    return dict(count_ms=o[0], generate_ms=o[1], sort_ms=o[2], copy_out_ms=o[3], total_ms=o[4], pairs=int(o[5]), sort_passes=int(o[6]),
                key_bytes=int(o[7]))


# --------------------------------------------------------------------------- spectrogram / melspectrogram / mfcc (DSP.spectrogram, src/mel.jl)
class Spectrogram:
    """DSP.Periodograms.Spectrogram: ``power`` ((nfft÷2+1) × frames), ``freq`` and ``time``."""

    def __init__(self, power, freq, time):
        self.power, self.freq, self.time = power, freq, time


class MelSpectrogram:
    """src/mel.jl MelSpectrogram: ``power`` (nmels × frames), ``mels`` and ``time``."""

    def __init__(self, power, mels, time):
        self.power, self.mels, self.time = power, mels, time


class MFCC:
    """src/mel.jl MFCC: ``mfcc`` (nmfcc × frames), ``number`` (1:nmfcc) and ``time``."""

    def __init__(self, mfcc, number, time):
        self.mfcc, self.number, self.time = mfcc, number, time


class Periodogram:
    """DSP.Periodograms.Periodogram: ``power`` (nfft÷2+1 values one-sided, nfft two-sided) and ``freq``."""

    def __init__(self, power, freq):
        self.power, self.freq = power, freq


def freq(M):
    """DSP.freq: the frequencies of a Spectrogram or Periodogram, the mels of a MelSpectrogram, the coefficient numbers of an MFCC."""
    return M.freq if isinstance(M, (Spectrogram, Periodogram)) else (M.mels if isinstance(M, MelSpectrogram) else M.number)


def time(M):
    """Base.time of a time-frequency representation: the frame centres."""
    return M.time


def _wide(x):
    """Julia's promotion of a mel argument: Python floats / np.float64 are Float64; ints and np.float32 stay Float32."""
    return isinstance(x, (float, np.floating)) and not isinstance(x, (np.float32, np.float16))


def nextfastfft(n):
    """DSP.nextfastfft: the smallest 2·3·5·7-smooth integer >= n."""
    out = C.c_int64(0)
    check(lib().lpvs_nextfastfft(int(n), C.byref(out)))
    return int(out.value)


def fft_frequencies(fs, nfft):
    """src/mel.jl: LinRange(0f0, fs/2f0, nfft>>1 + 1) (Float64 when fs is)."""
    dt = np.float64 if _wide(fs) else np.float32
    nb = (int(nfft) >> 1) + 1
    stop = dt(dt(fs) / dt(2))
    t = np.arange(nb) / max(nb - 1, 1)
    return ((1 - t) * 0.0 + t * np.float64(stop)).astype(dt)


def hz_to_mel(frequencies):
    """src/mel.jl:38-53 (Slaney): linear below 1 kHz, logarithmic above; Float32 constants, Float64 inputs widen."""
    f = np.atleast_1d(np.asarray(frequencies))
    dt = np.float64 if f.dtype == np.float64 else np.float32
    f = f.astype(dt)
    f_sp = np.float32(200) / np.float32(3)
    min_log_hz = np.float32(1000)
    min_log_mel = min_log_hz / f_sp
    logstep = np.float32(np.log(np.float64(np.float32(6.4)))) / np.float32(27)
    mels = (f - dt(0)) / dt(f_sp)
    hi = f >= min_log_hz
    mels[hi] = dt(min_log_mel) + np.log((f[hi] / dt(min_log_hz)).astype(np.float64)).astype(dt) / dt(logstep)
    return mels


def mel_to_hz(mels):
    """src/mel.jl:56-71, the inverse of :func:`hz_to_mel`."""
    m = np.atleast_1d(np.asarray(mels))
    dt = np.float64 if m.dtype == np.float64 else np.float32
    m = m.astype(dt)
    f_sp = np.float32(200) / np.float32(3)
    min_log_hz = np.float32(1000)
    min_log_mel = min_log_hz / f_sp
    logstep = np.float32(np.log(np.float64(np.float32(6.4)))) / np.float32(27)
    f = dt(0) + dt(f_sp) * m
    hi = m >= min_log_mel
    f[hi] = dt(min_log_hz) * np.exp((dt(logstep) * (m[hi] - dt(min_log_mel))).astype(np.float64)).astype(dt)
    return f


def _scalar_mel(x):
    return hz_to_mel(np.float64(x) if _wide(x) else np.float32(x))[0]


def mel_frequencies(nmels=128, fmin=np.float32(0), fmax=np.float32(11025)):
    """src/mel.jl:73-79: nmels points equally spaced in mel between fmin and fmax, in Hz."""
    lo, hi = _scalar_mel(fmin), _scalar_mel(fmax)
    dt = np.float64 if (lo.dtype == np.float64 or hi.dtype == np.float64) else np.float32
    t = np.arange(nmels) / max(nmels - 1, 1)
    return mel_to_hz(((1 - t) * np.float64(lo) + t * np.float64(hi)).astype(dt))


def mel(fs, nfft, nmels=128, fmin=np.float32(0), fmax=None):
    """src/mel.jl:99-113: the Float32 nmels × (nfft>>1 + 1) filterbank (Slaney mel scale, area-normalised triangles), computed by the
    library on the host in the reference's precision (Float64 where fs / fmin / fmax are)."""
    if fmax is None:
        fmax = float(fs) / 2 if _wide(fs) else np.float32(np.float32(fs) / np.float32(2))
    nfft, nmels = int(nfft), int(nmels)
    W = np.empty((nmels, (nfft >> 1) + 1), dtype=np.float32, order="F")
    wide = (1 if _wide(fs) else 0) | (2 if _wide(fmin) else 0) | (4 if _wide(fmax) else 0)
    check(lib().lpvs_mel_filterbank(float(fs), nfft, nmels, float(fmin), float(fmax), wide, out_ptr(W)))
    return W


def dct_matrix(nfilters, ninput):
    """src/mel.jl dct_matrix: Float32 rows cos(i (1:2:2ninput) π / 2ninput) · sqrt(2/ninput), i = 1 … nfilters (no DC row)."""
    D = np.empty((int(nfilters), int(ninput)), dtype=np.float32, order="F")
    check(lib().lpvs_dct_matrix(int(nfilters), int(ninput), out_ptr(D)))
    return D


def _stft_input(s):
    """(keepalive, pointer, length, f32, device index or None) of a real signal."""
    if _is_torch(s):
        if s.is_complex():
            raise ValueError("spectrogram: the signal must be real (the two-sided spectrogram of a complex signal is not built)")
        f32 = s.dtype == __import__("torch").float32
    else:
        a = np.asarray(s)
        if np.iscomplexobj(a):
            raise ValueError("spectrogram: the signal must be real (the two-sided spectrogram of a complex signal is not built)")
        f32 = a.dtype == np.float32
    keep, ptr, L = (as_f32 if f32 else as_f64)(s)
    dev = s.device.index if _is_torch(s) and s.is_cuda else None
    return keep, ptr, L, f32, dev


def _stft(kind, s, n, noverlap, nfft, fs, window, W=None, D=None, device=0):
    keep, ptr, L, f32, dev = _stft_input(s)
    n = L >> 3 if n is None else int(n)
    noverlap = n >> 1 if noverlap is None else int(noverlap)
    nfft = nextfastfft(n) if nfft is None else int(nfft)
    if noverlap < 0 or noverlap >= n:
        raise _lib.DomainError(f"noverlap must satisfy 0 <= noverlap < n (noverlap = {noverlap}, n = {n})")   # DSP.arraysplit
    if nfft < n:
        raise ValueError(f"nfft must be >= n (nfft = {nfft}, n = {n})")
    dt = np.float32 if f32 else np.float64
    win = None
    if window is not None:
        win = np.ascontiguousarray(np.asarray(window(n) if callable(window) else window, dtype=np.float64).ravel())
        if len(win) != n:
            raise ValueError(f"window has {len(win)} values, the frames {n}")
        win = win.astype(dt)
    nmels = 0 if W is None else W.shape[0]
    nmfcc = 0 if D is None else D.shape[0]
    rows = {_lib.STFT_POWER: nfft // 2 + 1, _lib.STFT_MEL: nmels, _lib.STFT_MFCC: nmfcc}[kind]
    fn = lib().lpvs_stft_f32 if f32 else lib().lpvs_stft_f64
    device = dev if dev is not None else device
    wp = out_ptr(win) if win is not None else None
    Wp = out_ptr(W) if W is not None else None
    Dp = out_ptr(D) if D is not None else None
    k = C.c_int64(0)
    args = (kind, ptr, L, n, noverlap, nfft, float(fs), wp, Wp, nmels, Dp, nmfcc, int(device))
    check(fn(*args, None, 0, C.byref(k)))                                     # count only
    k = int(k.value)
    if dev is not None:
        import torch
        o = torch.empty((k, rows), dtype=torch.float32 if f32 else torch.float64, device=s.device)
        check(fn(*args, C.c_void_p(o.data_ptr()), k * rows, C.byref(C.c_int64(0))))
        out = o.T                                                              # rows × frames, column-major storage
    else:
        out = np.empty((rows, k), dtype=dt, order="F")
        check(fn(*args, out_ptr(out), k * rows, C.byref(C.c_int64(0))))
    del keep
    tm = (n / 2 + np.arange(k) * (n - noverlap)) / fs
    return out, nfft, tm


def spectrogram(s, n=None, noverlap=None, nfft=None, fs=1, window=None, device=0):
    """DSP.spectrogram of a real signal: the one-sided power of the frames of DSP.arraysplit(s, n, noverlap), windowed and
    zero-padded to nfft (default nextfastfft(n)); n defaults to len(s)>>3, noverlap to n>>1.  ``window`` is a function of n, a vector
    or None.  Torch device tensors give device tensors, host arrays numpy arrays (f32 in, f32 out)."""
    P, nfft, tm = _stft(_lib.STFT_POWER, s, n, noverlap, nfft, fs, window, device=device)
    return Spectrogram(P, np.arange(nfft // 2 + 1) * fs / nfft, tm)


def _mel_axis(nmels, fmin, fmax):
    lo, hi = _scalar_mel(fmin), _scalar_mel(fmax)
    dt = np.float64 if (lo.dtype == np.float64 or hi.dtype == np.float64) else np.float32
    return np.linspace(np.float64(lo), np.float64(hi), int(nmels)).astype(dt)


def melspectrogram(s, n=None, *args, fs=1, nmels=128, fmin=np.float32(0), fmax=None, window=hanning, device=0, **kwargs):
    """src/mel.jl:133-143.  ``melspectrogram(s, n, noverlap; fs, nmels, fmin, fmax, window=hanning, nfft)``: the Float32 filterbank
    mel(fs, 2·size(S.power,1) - 1) applied to the spectrogram's power (for odd nfft its grid runs to exactly fs/2, the reference's quirk),
    fused into the STFT on the device.  ``melspectrogram(S::Spectrogram; fs, nmels, fmin, fmax)`` projects an existing spectrogram."""
    if fmax is None:
        fmax = float(fs) / 2 if _wide(fs) else np.float32(np.float32(fs) / np.float32(2))
    if isinstance(s, Spectrogram):
        P = s.power
        nbins, frames = int(P.shape[0]), int(P.shape[1])
        W = mel(fs, 2 * nbins - 1, nmels=nmels, fmin=fmin, fmax=fmax)
        if _is_torch(P) and P.is_cuda:
            import torch
            f32 = P.dtype == torch.float32
            src = P.T.contiguous()                                             # frames × nbins row-major = nbins × frames column-major
            torch.cuda.current_stream(src.device).synchronize()
            o = torch.empty((frames, int(nmels)), dtype=src.dtype, device=src.device)
            fn = lib().lpvs_mel_project_f32 if f32 else lib().lpvs_mel_project_f64
            check(fn(C.c_void_p(src.data_ptr()), nbins, frames, out_ptr(W), int(nmels), src.device.index, C.c_void_p(o.data_ptr())))
            out = o.T
        else:
            f32 = isinstance(P, np.ndarray) and P.dtype == np.float32
            dt = np.float32 if f32 else np.float64
            src = np.asfortranarray(np.asarray(P, dtype=dt))
            out = np.empty((int(nmels), frames), dtype=dt, order="F")
            fn = lib().lpvs_mel_project_f32 if f32 else lib().lpvs_mel_project_f64
            check(fn(out_ptr(src), nbins, frames, out_ptr(W), int(nmels), int(device), out_ptr(out)))
        return MelSpectrogram(out, _mel_axis(nmels, fmin, fmax), s.time)
    noverlap = args[0] if args else kwargs.pop("noverlap", None)
    nfft = kwargs.pop("nfft", None)
    if kwargs:
        raise TypeError(f"melspectrogram: unknown keywords {sorted(kwargs)}")
    L_ = len(s) if not _is_torch(s) else s.numel()
    n_ = L_ >> 3 if n is None else int(n)
    nfft_ = nextfastfft(n_) if nfft is None else int(nfft)
    W = mel(fs, 2 * (nfft_ // 2 + 1) - 1, nmels=nmels, fmin=fmin, fmax=fmax)
    out, _, tm = _stft(_lib.STFT_MEL, s, n_, noverlap, nfft_, fs, window, W=W, device=device)
    return MelSpectrogram(out, _mel_axis(nmels, fmin, fmax), tm)


def mfcc(s, *args, nmfcc=20, nmels=128, window=hanning, fs=1, fmin=np.float32(0), fmax=None, device=0, **kwargs):
    """src/mel.jl:159-172: dct_matrix(nmfcc, nmels) * power(melspectrogram(s, args...)), every column divided by its 2-norm.  As the
    reference: no log before the DCT, the DC row is skipped, and a zero column gives 0/0 = NaN."""
    if nmfcc >= nmels:
        raise ValueError("number of mfcc components should be less than the number of mel frequency bins")
    if fmax is None:
        fmax = float(fs) / 2 if _wide(fs) else np.float32(np.float32(fs) / np.float32(2))
    n = args[0] if args else kwargs.pop("n", None)
    noverlap = args[1] if len(args) > 1 else kwargs.pop("noverlap", None)
    nfft = kwargs.pop("nfft", None)
    if kwargs:
        raise TypeError(f"mfcc: unknown keywords {sorted(kwargs)}")
    L_ = len(s) if not _is_torch(s) else s.numel()
    n_ = L_ >> 3 if n is None else int(n)
    nfft_ = nextfastfft(n_) if nfft is None else int(nfft)
    W = mel(fs, 2 * (nfft_ // 2 + 1) - 1, nmels=nmels, fmin=fmin, fmax=fmax)
    D = dct_matrix(nmfcc, nmels)
    out, _, tm = _stft(_lib.STFT_MFCC, s, n_, noverlap, nfft_, fs, window, W=W, D=D, device=device)
    return MFCC(out, np.arange(1, int(nmfcc) + 1), tm)


def stft_last_timing():
    """HIP-event times (ms) and plan of this thread's last spectrogram / melspectrogram / mfcc / welch_pgram / periodogram call.
    ``sum_chain`` is the longest chain of dependent additions behind one bin of a frame average (D of DESIGN.md §4.10) and ``slabs``
    the partial-sum slabs it was built from; both are 0 after the other calls."""
    o = np.zeros(11)
    check(lib().lpvs_stft_last_timing(out_ptr(o), 11))
    return dict(fft_ms=o[0], copy_out_ms=o[1], total_ms=o[2], frames=int(o[3]), path=int(o[4]), fft_length=int(o[5]),
                pairs_per_workgroup=int(o[6]), rows=int(o[7]), setup_ms=o[8], sum_chain=int(o[9]), slabs=int(o[10]))


# --------------------------------------------------------------------------- welch_pgram / periodogram (DSP.jl), compress / heatmap
# (src/plotting.jl:8-47: the numbers of plot_periodogram, plot_spectrogram and the MelSpectrogram recipe; csrc/melspec.hip, csrc/compress.hip)
def _welch(s, n, noverlap, nfft, fs, window, onesided, device):
    keep, ptr, L, f32, dev = _stft_input(s)
    n = L >> 3 if n is None else int(n)
    noverlap = n >> 1 if noverlap is None else int(noverlap)
    nfft = nextfastfft(n) if nfft is None else int(nfft)
    if n < 1 or L < n:
        raise _lib.DomainError(f"the signal ({L} samples) holds no frame of n = {n} samples: the mean over no frame is undefined")
    if noverlap < 0 or noverlap >= n:
        raise _lib.DomainError(f"noverlap must satisfy 0 <= noverlap < n (noverlap = {noverlap}, n = {n})")   # DSP.arraysplit
    if nfft < n:
        raise ValueError(f"nfft must be >= n (nfft = {nfft}, n = {n})")
    dt = np.float32 if f32 else np.float64
    win = None
    if window is not None:
        win = np.ascontiguousarray(np.asarray(window(n) if callable(window) else window, dtype=np.float64).ravel())
        if len(win) != n:
            raise ValueError(f"window has {len(win)} values, the frames {n}")
        win = win.astype(dt)
    rows = nfft // 2 + 1 if onesided else nfft
    fn = lib().lpvs_welch_f32 if f32 else lib().lpvs_welch_f64
    device = dev if dev is not None else device
    wp = out_ptr(win) if win is not None else None
    k = C.c_int64(0)
    args = (ptr, L, n, noverlap, nfft, float(fs), wp, 1 if onesided else 0, int(device))
    if dev is not None:
        import torch
        out = torch.empty(rows, dtype=torch.float32 if f32 else torch.float64, device=s.device)
        check(fn(*args, C.c_void_p(out.data_ptr()), C.byref(k)))
    else:
        out = np.empty(rows, dtype=dt)
        check(fn(*args, out_ptr(out), C.byref(k)))
    del keep
    f = np.arange(nfft // 2 + 1) * fs / nfft if onesided else np.fft.fftfreq(nfft, 1.0 / fs)
    return Periodogram(out, f)


def welch_pgram(s, n=None, noverlap=None, onesided=True, nfft=None, fs=1, window=None, device=0):
    """DSP.welch_pgram of a real signal: the mean over the frames of DSP.arraysplit(s, n, noverlap) of their power (the columns of
    :func:`spectrogram`), summed on the device without the power matrix.  n defaults to len(s)>>3, noverlap to n>>1, nfft to
    nextfastfft(n).  ``onesided=False`` gives all nfft bins (bins k and nfft-k hold the same, undoubled value).  A signal shorter than
    one frame raises DomainError.  Torch device tensors give device tensors, host arrays numpy arrays (f32 in, f32 out)."""
    return _welch(s, n, noverlap, nfft, fs, window, onesided, device)


def periodogram(s, onesided=True, nfft=None, fs=1, window=None, device=0):
    """DSP.periodogram of a real signal: the one-frame case of :func:`welch_pgram` (n = len(s), nfft = nextfastfft(len(s)))."""
    L = s.numel() if _is_torch(s) else np.asarray(s).size
    return _welch(s, L, 0, nfft, fs, window, onesided, device)


def _quantile_pair(q):
    """compress's q (src/plotting.jl:39-44): a number q -> (q', 1-q') with q' = q < 0.5 ? q : 1-q; a pair -> (min, max)."""
    if isinstance(q, (int, float, np.integer, np.floating)):
        q = float(q)
        q = q if q < 0.5 else 1 - q
        q = (q, 1 - q)
    else:
        q = tuple(float(v) for v in q)
        if len(q) < 1:
            raise ValueError("compress: q must be a number or a non-empty collection of numbers")
        q = (min(q), max(q))
    if not (0 <= q[0] <= 1 and 0 <= q[1] <= 1):
        raise ValueError(f"compress: quantile levels must lie in [0, 1], got {q}")       # Julia's quantile: ArgumentError
    return q


def _compress(x, q, take_log, device=0):
    qlo, qhi = _quantile_pair(q)
    th = np.zeros(2)
    if _is_torch(x) and x.is_cuda:
        import torch
        if x.is_complex() or x.dim() not in (1, 2):
            raise ValueError("compress: x must be a real vector or matrix")
        v = x if x.dim() == 2 else x.reshape(-1, 1)
        if v.dtype not in (torch.float32, torch.float64):
            v = v.to(torch.float64)
        rows, cols = int(v.shape[0]), int(v.shape[1])
        if rows * cols == 0:
            raise _lib.DomainError("compress: the quantiles of an empty collection are undefined")
        if not ((rows == 1 or v.stride(0) == 1) and (cols == 1 or v.stride(1) >= rows)):
            v = v.T.contiguous().T                                             # column-major copy
        ld = rows if cols == 1 else int(v.stride(1))
        f32 = v.dtype == torch.float32
        torch.cuda.current_stream(v.device).synchronize()
        o = torch.empty((cols, rows), dtype=v.dtype, device=v.device)
        fn = lib().lpvs_compress_f32 if f32 else lib().lpvs_compress_f64
        check(fn(C.c_void_p(v.data_ptr()), rows, cols, ld, int(take_log), qlo, qhi, v.device.index, C.c_void_p(o.data_ptr()), rows, out_ptr(th)))
        out = o.T if x.dim() == 2 else o.reshape(-1)
        return out, (float(th[0]), float(th[1]))
    if hasattr(x, "detach") and hasattr(x, "numpy"):
        x = x.detach().numpy()
    a = np.asarray(x)
    if np.iscomplexobj(a) or a.ndim not in (1, 2):
        raise ValueError("compress: x must be a real vector or matrix")
    dt = np.float32 if a.dtype == np.float32 else np.float64
    v = a.astype(dt, copy=False)
    v = v if v.ndim == 2 else v.reshape(-1, 1)
    rows, cols = v.shape
    if rows * cols == 0:
        raise _lib.DomainError("compress: the quantiles of an empty collection are undefined")
    isz = v.itemsize
    if not ((rows == 1 or v.strides[0] == isz) and (cols == 1 or (v.strides[1] % isz == 0 and v.strides[1] // isz >= rows))):
        v = np.asfortranarray(v)
    ld = rows if cols == 1 else v.strides[1] // isz
    out = np.empty((rows, cols), dtype=dt, order="F")
    fn = lib().lpvs_compress_f32 if dt is np.float32 else lib().lpvs_compress_f64
    check(fn(C.c_void_p(v.ctypes.data), rows, cols, ld, int(take_log), qlo, qhi, int(device), out_ptr(out), rows, out_ptr(th)))
    return (out if a.ndim == 2 else out.reshape(-1)), (float(th[0]), float(th[1]))


def compress(x, q, device=0):
    """src/plotting.jl:38-47: ``clamp.(x, quantile(vec(x), q)...)`` with q a number (-> (q', 1-q'), q' = q < 0.5 ? q : 1-q) or a pair
    (-> (min, max)); Julia's default quantile definition.  The order statistics come from an exact radix select on the device, so the
    thresholds equal those of a sort.  x: a real vector or matrix, host array or torch device tensor (a column-major view such as
    ``power[1:, :]`` is read in place).  float32 in gives float32 out: the order statistics are the float values, the interpolation runs
    in double and a clamped element is the threshold rounded to float (the reference would widen the whole matrix to Float64).  An
    empty x or a NaN in it raises DomainError, as Julia's quantile throws."""
    return _compress(x, q, 0, device)[0]


def compress_thresholds(x, q, take_log=False, device=0):
    """(clamped matrix, (lower, upper) thresholds) of :func:`compress`, of ``log(x)`` when take_log (the log is fused on the device)."""
    return _compress(x, q, 1 if take_log else 0, device)


def heatmap(S, compression=(0.005, 1), device=0):
    """The numbers of the reference's heat-map recipes (src/plotting.jl:15-36): for a Spectrogram ``(time, freq[1:], z)``, for a
    MelSpectrogram ``(time, mel_to_hz(mels)[1:], z)``, z = compress(log(power)[1:, :], compression) -- log, selection and clamp on the
    device, row 0 skipped in place.  A zero power gives -Inf and is legal; a NaN (or negative) power raises DomainError."""
    if isinstance(S, Spectrogram):
        axis = S.freq[1:]
    elif isinstance(S, MelSpectrogram):
        axis = mel_to_hz(S.mels)[1:]
    else:
        raise TypeError("heatmap: a Spectrogram or a MelSpectrogram is needed")
    z, _ = _compress(S.power[1:, :], compression, 1, device)
    return S.time, axis, z


_LOMB_NORMALIZATIONS = {"standard": 0, "psd": 1}


def _lomb_signals(y):
    """Signals as what the library reads -- N x ns column-major -- and (N, ns, whether the caller gave one vector)."""
    y = _f64_arg(y)
    if _lib.is_device_array(y):
        single = y.dim() == 1
        N, ns = int(y.shape[0]), 1 if single else int(y.shape[1])
        return (y if single else y.t().contiguous()), N, ns, single      # (ns, N) row-major = N x ns column-major
    ya = _host(y)
    single = ya.ndim == 1
    ya = ya.reshape(ya.shape[0], -1)
    return np.asfortranarray(ya), ya.shape[0], ya.shape[1], single


def lombscargle(y, t, f=None, W=None, fit_mean=True, center_data=True, normalization="standard", path="auto", device=0, coef=False, return_sums=False, nterms=1):
    """Generalised Lomb-Scargle periodogram of non-uniformly sampled signals (extension; the floating-mean form of Zechmeister &
    Kürster 2009): every frequency is fitted on its own, ``y ≈ c + a cos 2πft + b sin 2πft`` in weighted least squares.

    ``y``: (N,) or (N, ns) signals sharing the times ``t``; ``f``: frequencies in cycles per unit of ``t`` (``None``:
    ``default_freqs(t)``); ``W``: non-negative weights (``None``: ones), normalised to sum 1.  ``fit_mean``: the constant is fitted
    along with the sinusoid at every frequency; ``center_data``: the weighted mean is removed first.  ``normalization``:
    ``"standard"`` (``p / YY`` in [0, 1]) or ``"psd"`` (``p N / 2``: with unit weights the classical unnormalised periodogram, what
    ``scipy.signal.lombscargle`` returns).  ``path``: ``"auto"``, ``"direct"`` (any frequency grid) or ``"nufft"`` (non-uniform FFTs in
    blocks of modes, for grids that are an arithmetic progression up to rounding; ValueError otherwise).  Phases are those of the exact
    products ``f t``.  Frequencies where the fit is degenerate (``f = 0``, the Nyquist alias of a uniform record) give 0.

    Returns a :class:`Periodogram` (``power``: (Nf,) or (Nf, ns)); with ``coef=True`` also ``(a, b, c)``, with ``return_sums=True``
    also the raw sums as a dict (with ``"mean"``: the weighted means as the device formed them).  A constant signal has standard power 0
    (a ``YY`` within rounding of 0 counts as 0).  Float32 inputs are widened; a non-finite input, a negative weight or a zero weight sum raise
    ValueError.

    ``nterms=K`` in 2 .. 6 fits ``K`` harmonics per frequency, ``y ≈ c + Σ_h a_h cos 2πhft + b_h sin 2πhft`` (astropy's ``nterms``; for
    signals that are periodic but not sinusoidal): one ``sincospi`` per (sample, frequency) and complex rotations for the harmonics, the
    ``2K × 2K`` normal equations factored per frequency on the device (csrc/lomb_terms.hip; include/lpvspectral.h g7).  Only direct sums:
    ``path="nufft"`` raises ValueError (the transforms are not implemented for several terms), ``"auto"`` and ``"direct"`` run the
    direct sums.  ``coef=True`` then gives ``(a, b, c)`` with ``a``, ``b`` of shape (K, Nf[, ns]) and ``c`` of shape (Nf[, ns]);
    ``return_sums=True`` a dict with ``"C"``, ``"S"``: (2K, Nf) (harmonics 1 .. 2K), ``"YC"``, ``"YS"``: (ns, K, Nf), and ``"Y"``,
    ``"YY"``, ``"mean"``.  A frequency where a pivot of the factorisation is not above 2^-40 is degenerate and gives 0
    (:func:`lombscargle_terms_last_timing` counts them).  ``false_alarm_probability`` / ``false_alarm_level``, the windowed estimators
    and :func:`lombscargle_bootstrap` stay single-term."""
    if path not in _EVAL_PATHS:
        raise ValueError(f"path: unknown value {path!r} (known: {sorted(_EVAL_PATHS)})")
    if normalization not in _LOMB_NORMALIZATIONS:
        raise ValueError(f"normalization: unknown value {normalization!r} (known: {sorted(_LOMB_NORMALIZATIONS)})")
    if int(nterms) != nterms or not 1 <= int(nterms) <= 6:
        raise ValueError(f"nterms must be an integer in 1 .. 6, got {nterms!r}")
    if int(nterms) > 1:
        if path == "nufft":
            raise ValueError(f'path="nufft": the transforms are not implemented for several terms (nterms = {int(nterms)}); use "auto" or "direct"')
        return _lombscargle_terms(y, t, f, W, fit_mean, center_data, normalization, device, coef, return_sums, int(nterms))
    fa = np.ascontiguousarray(np.ravel(_host(default_freqs(t) if f is None else f)).astype(np.float64))
    Nf = len(fa)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    power = np.zeros((Nf, ns), order="F")
    co = np.zeros((3, ns, Nf)) if coef else None                           # [plane][signal][frequency] = planes of Nf x ns column-major
    sums = np.zeros((4 + 2 * ns) * Nf + 3 * ns) if return_sums else None
    check(lib().lpvs_lombscargle_f64(py, ns, pt, N, pw, out_ptr(fa), Nf, int(bool(fit_mean)), int(bool(center_data)), _LOMB_NORMALIZATIONS[normalization],
                                     _EVAL_PATHS[path], int(device), out_ptr(power), out_ptr(co) if coef else None, out_ptr(sums) if return_sums else None))
    res = [Periodogram(power[:, 0].copy() if single else power, fa)]
    if coef:
        res.append(tuple((co[i, 0].copy() if single else np.asfortranarray(co[i].T)) for i in range(3)))
    if return_sums:
        nr = (4 + 2 * ns) * Nf
        rows, mom, mean = sums[:nr].reshape(4 + 2 * ns, Nf), sums[nr:nr + 2 * ns].reshape(ns, 2), sums[nr + 2 * ns:]
        res.append({"C": rows[0], "S": rows[1], "C2": rows[2], "S2": rows[3], "YC": rows[4::2], "YS": rows[5::2], "Y": mom[:, 0], "YY": mom[:, 1],
                    "mean": mean})
    return res[0] if len(res) == 1 else tuple(res)


def _lombscargle_terms(y, t, f, W, fit_mean, center_data, normalization, device, coef, return_sums, nterms):
    """:func:`lombscargle` with ``nterms`` harmonics through ``lpvs_lombscargle_terms_f64`` (``nterms=1`` is admitted here, for tests: the
    public function keeps its own entry for one term)."""
    K = int(nterms)
    fa = np.ascontiguousarray(np.ravel(_host(default_freqs(t) if f is None else f)).astype(np.float64))
    Nf = len(fa)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    nrow = max(4 * K + 2 * K * ns, 0)
    power = np.zeros((Nf, ns), order="F")
    co = np.zeros((max(2 * K + 1, 1), ns, Nf)) if coef else None           # [plane][signal][frequency] = planes of Nf x ns column-major
    sums = np.zeros(nrow * Nf + 3 * ns) if return_sums else None
    check(lib().lpvs_lombscargle_terms_f64(py, ns, pt, N, pw, out_ptr(fa), Nf, K, int(bool(fit_mean)), int(bool(center_data)), _LOMB_NORMALIZATIONS[normalization],
                                           int(device), out_ptr(power), out_ptr(co) if coef else None, out_ptr(sums) if return_sums else None))
    res = [Periodogram(power[:, 0].copy() if single else power, fa)]
    if coef:
        shaped = (lambda x: x[..., 0, :].copy()) if single else (lambda x: np.ascontiguousarray(np.swapaxes(x, -1, -2)))
        res.append((shaped(co[0:2 * K:2]), shaped(co[1:2 * K:2]), shaped(co[2 * K])))
    if return_sums:
        nr = nrow * Nf
        rows, mom, mean = sums[:nr].reshape(nrow, Nf), sums[nr:nr + 2 * ns].reshape(ns, 2), sums[nr + 2 * ns:]
        ycs = rows[4 * K:].reshape(ns, K, 2, Nf)
        res.append({"C": rows[0:4 * K:2], "S": rows[1:4 * K:2], "YC": ycs[:, :, 0], "YS": ycs[:, :, 1], "Y": mom[:, 0], "YY": mom[:, 1], "mean": mean})
    return res[0] if len(res) == 1 else tuple(res)


def lombscargle_terms_last_timing():
    """Plan and timing of the calling thread's last :func:`lombscargle` with ``nterms > 1``: the terms, the signals and the accumulators
    per thread of the sums kernel, the slabs, the degenerate frequencies, milliseconds per phase."""
    o = np.zeros(10)
    check(lib().lpvs_lombscargle_terms_last_timing(out_ptr(o), 10))
    return {"nterms": int(o[0]), "ts": int(o[1]), "slabs": int(o[2]), "degenerate": int(o[3]), "moments_ms": float(o[4]), "sums_ms": float(o[5]),
            "epilogue_ms": float(o[6]), "copy_ms": float(o[7]), "total_ms": float(o[8]), "accumulators": int(o[9])}


def lombscargle_last_timing():
    """Plan and timing of the calling thread's last :func:`lombscargle`: the path taken, the blocks per family and the fine grid of the
    transforms, the degenerate frequencies, the slabs of the direct sums, milliseconds per phase."""
    o = np.zeros(12)
    check(lib().lpvs_lombscargle_last_timing(out_ptr(o), 12))
    return {"path": {1: "direct", 2: "nufft"}.get(int(o[0]), "none"), "blocks": (int(o[1]), int(o[2])), "nf": int(o[3]), "degenerate": int(o[4]),
            "slabs": int(o[5]), "moments_ms": float(o[6]), "sums_ms": float(o[7]), "epilogue_ms": float(o[8]), "copy_ms": float(o[9]),
            "total_ms": float(o[10]), "twin": bool(o[11])}


def time_windows(t, lo, hi, device=0):
    """The index ranges of the time intervals ``[lo[w], hi[w]]`` in a non-decreasing ``t`` (host array or device tensor): ``(starts,
    counts)`` with ``starts[w] = #{t < lo[w]}`` and ``counts[w] = #{t <= hi[w]} - starts[w]`` -- ``np.searchsorted`` left and right --
    by one binary search per edge on the device.  A ``t`` that decreases somewhere, or a non-finite value, raises ValueError."""
    la, ha = (np.ascontiguousarray(np.ravel(_host(v)).astype(np.float64)) for v in (lo, hi))
    if len(la) != len(ha):
        raise ValueError(f"lo has {len(la)} values, hi has {len(ha)}")
    kt, pt, N = as_f64(_f64_arg(t))
    starts, counts = np.zeros(len(la), dtype=np.int64), np.zeros(len(la), dtype=np.int64)
    check(lib().lpvs_time_windows_f64(pt, N, out_ptr(la), out_ptr(ha), len(la), int(device), out_ptr(starts), out_ptr(counts)))
    del kt
    return starts, counts


_LOMB_TAPERS = {"rect": 0, "hanning": 1}


def _lomb_window_list(t, N, n, noverlap, width, hop, windows, device):
    """(starts, counts, lo, hi) of the one window form that was given."""
    forms = [n is not None or noverlap is not None, width is not None or hop is not None, windows is not None]
    if sum(forms) > 1:
        raise ValueError("give the windows in one form: n (noverlap), width (hop) or windows=(starts, counts, lo, hi)")
    if windows is not None:
        if len(windows) != 4:
            raise ValueError("windows: (starts, counts, lo, hi) is needed")
        starts, counts = (np.ascontiguousarray(np.ravel(np.asarray(v)).astype(np.int64)) for v in windows[:2])
        lo, hi = (np.ascontiguousarray(np.ravel(_host(v)).astype(np.float64)) for v in windows[2:])
        if not len(starts) == len(counts) == len(lo) == len(hi):
            raise ValueError("windows: starts, counts, lo and hi differ in length")
        return starts, counts, lo, hi
    if forms[1]:
        if width is None:
            raise ValueError("hop needs width")
        width = float(width)
        hop = width / 2 if hop is None else float(hop)
        if not (width > 0 and hop > 0 and np.isfinite(width) and np.isfinite(hop)):
            raise ValueError(f"width and hop must be positive and finite (width = {width}, hop = {hop})")
        ends = _host(t[[0, -1]] if _is_torch(t) else np.asarray(t)[[0, -1]])
        first, last = np.float64(ends[0]), np.float64(ends[1])
        nwin = int(np.floor((last - first) / hop)) + 1
        lo = first + np.arange(nwin + 1, dtype=np.float64) * np.float64(hop)      # (one more, then cut: the quotient above is rounded)
        lo = lo[lo <= last]
        hi = lo + np.float64(width)
        starts, counts = time_windows(t, lo, hi, device)
        return starts, counts, lo, hi
    n = N >> 3 if n is None else int(n)
    noverlap = n >> 1 if noverlap is None else int(noverlap)
    if n < 1 or N < n:
        raise _lib.DomainError(f"the record ({N} samples) holds no window of n = {n} samples")
    if noverlap < 0 or noverlap >= n:
        raise _lib.DomainError(f"noverlap must satisfy 0 <= noverlap < n (noverlap = {noverlap}, n = {n})")
    from .windows import _offsets
    starts = np.ascontiguousarray(_offsets(N, n, noverlap), dtype=np.int64)
    th = np.ravel(_host(t))
    return starts, np.full(len(starts), n, dtype=np.int64), th[starts].copy(), th[starts + n - 1].copy()


def _lomb_windows(y, t, f, n, noverlap, width, hop, windows, window, W, fit_mean, center_data, normalization, coef, average, device):
    if normalization not in _LOMB_NORMALIZATIONS:
        raise ValueError(f"normalization: unknown value {normalization!r} (known: {sorted(_LOMB_NORMALIZATIONS)})")
    if window is hanning:
        taper = _LOMB_TAPERS["hanning"]
    elif window is rect:
        taper = _LOMB_TAPERS["rect"]
    else:
        raise ValueError("window: hanning or rect (the taper is evaluated from the sample times, not from a vector of n values)")
    if coef and average:
        raise ValueError("coef: the coefficients of an average over windows are not defined")
    fa = np.ascontiguousarray(np.ravel(_host(default_freqs(t) if f is None else f)).astype(np.float64))
    Nf = len(fa)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    starts, counts, lo, hi = _lomb_window_list(t, N, n, noverlap, width, hop, windows, device)
    nwin = len(starts)
    if nwin == 0:
        raise ValueError("no window")
    power = np.zeros((ns, Nf) if average else (ns, nwin, Nf))               # [signal][window][frequency]: frequency fastest
    co = np.zeros((3, ns, nwin, Nf)) if coef else None
    empty = np.zeros(nwin, dtype=np.int32)
    check(lib().lpvs_lombscargle_windows_f64(py, ns, pt, N, pw, out_ptr(fa), Nf, out_ptr(starts), out_ptr(counts), out_ptr(lo), out_ptr(hi), nwin, taper,
                                             int(bool(fit_mean)), int(bool(center_data)), _LOMB_NORMALIZATIONS[normalization], int(bool(average)), int(device),
                                             out_ptr(power), out_ptr(co) if coef else None, out_ptr(empty)))
    del ky, kt, kw

    def shaped(a):                                                             # (ns, nwin, Nf) -> (Nf, nwin) or (Nf, nwin, ns)
        return np.ascontiguousarray(a[0].T) if single else np.ascontiguousarray(np.transpose(a, (2, 1, 0)))
    if average:
        return Periodogram(power[0].copy() if single else np.asfortranarray(power.T), fa)
    S = Spectrogram(shaped(power), fa, (lo + hi) / 2)
    S.counts, S.empty = counts, empty.astype(bool)
    return (S, tuple(shaped(co[i]) for i in range(3))) if coef else S


def lombscargle_spectrogram(y, t, f=None, n=None, noverlap=None, width=None, hop=None, windows=None, window=hanning, W=None, fit_mean=True,
                            center_data=True, normalization="standard", coef=False, device=0):
    """The non-uniform twin of :func:`spectrogram`: the :func:`lombscargle` estimate of every window of the record, all windows, all
    frequencies and all signals in one batched call (direct sums; csrc/lomb.hip).

    The windows are given in ONE of three forms (two together raise ValueError): ``n`` (``noverlap``): windows of n samples, the
    arithmetic of :class:`Windows2` (defaults ``n = len(y) >> 3``, ``noverlap = n >> 1``), with the time interval from the first to the
    last sample of the window (``t`` need not be sorted); ``width`` (``hop``, default ``width / 2``): windows of equal duration
    ``[t[0] + w hop, t[0] + w hop + width]`` as long as they begin in the record, their samples found by :func:`time_windows` (``t``
    sorted); ``windows=(starts, counts, lo, hi)``: explicit index ranges and time intervals -- they may overlap, leave gaps, differ in
    length, come in any order and be empty.  ``window``: ``hanning`` or ``rect``; the taper is evaluated from the sample TIMES,
    ``sin²(π (t - lo) / (hi - lo))``, and multiplies the weights ``W``.  Everything else as in :func:`lombscargle`, per window.

    Returns a :class:`Spectrogram`: ``power`` (Nf, nwin) or (Nf, nwin, ns), ``freq = f``, ``time = (lo + hi) / 2``, and the added
    attributes ``counts`` (samples per window) and ``empty`` (windows without samples or with weights that sum to 0: their columns are
    0).  With ``coef=True`` also ``(a, b, c)`` of the same shape.  A column has the same bits whether its window is computed alone or
    among others."""
    return _lomb_windows(y, t, f, n, noverlap, width, hop, windows, window, W, fit_mean, center_data, normalization, coef, False, device)


def lombscargle_welch(y, t, f=None, n=None, noverlap=None, width=None, hop=None, windows=None, window=hanning, W=None, fit_mean=True,
                      center_data=True, normalization="standard", device=0):
    """The non-uniform twin of :func:`welch_pgram`: the mean of the columns of :func:`lombscargle_spectrogram` over the windows that are
    not empty, added on the device in a fixed pairwise tree (0 if every window is empty).  Returns a :class:`Periodogram` (``power``:
    (Nf,) or (Nf, ns))."""
    return _lomb_windows(y, t, f, n, noverlap, width, hop, windows, window, W, fit_mean, center_data, normalization, False, True, device)


def lombscargle_windows_last_timing():
    """Plan and timing of the calling thread's last :func:`lombscargle_spectrogram` / :func:`lombscargle_welch`."""
    o = np.zeros(10)
    check(lib().lpvs_lombscargle_windows_last_timing(out_ptr(o), 10))
    return {"windows": int(o[0]), "empty": int(o[1]), "items": int(o[2]), "slab": int(o[3]), "degenerate": int(o[4]), "moments_ms": float(o[5]),
            "sums_ms": float(o[6]), "epilogue_ms": float(o[7]), "copy_ms": float(o[8]), "total_ms": float(o[9])}


# ---- weighted wavelet Z-transform (include/lpvspectral.h g8; csrc/wwz.hip) ------------------------------------------------------------------
WWZ_DECAY = 1.0 / (8.0 * np.pi ** 2)


class WWZ(Spectrogram):
    """The result of :func:`wwz`, laid out as a :class:`Spectrogram` (``power``, ``freq``, ``time``: :func:`heatmap` takes it as it is):
    ``power`` (standard, in [0, 1]), ``wwz`` (Foster's Z) and ``amplitude`` (his WWA): (Nf, Ntau) or (Nf, Ntau, ns); ``neff``,
    ``counts`` (samples in reach) and ``empty``: (Nf, Ntau); ``freq = f``, ``time = tau``, and the ``radius`` of every frequency."""

    def __init__(self, power, freq, time, wwz, amplitude, neff, counts, empty, radius):
        super().__init__(power, freq, time)
        self.wwz, self.amplitude, self.neff, self.counts, self.empty, self.radius = wwz, amplitude, neff, counts, empty, radius


def wwz_radius(f, c=WWZ_DECAY, wmin=1e-9):
    """How far a cell of :func:`wwz` reaches: the distance at which the weight ``exp(-c (2π f d)²)`` has fallen to ``wmin``,
    ``sqrt(log(1 / wmin) / c) / (2π f)`` in numpy doubles (``inf`` for ``wmin = 0``: every cell is the whole record).  The library
    takes radii and never a ``wmin``, so this expression IS the definition."""
    fa = np.asarray(_host(f), dtype=np.float64)
    wmin = np.float64(wmin)
    if not 0 <= wmin < 1:
        raise ValueError(f"wmin must lie in [0, 1), got {wmin}")
    if wmin == 0:
        return np.full(fa.shape, np.inf)
    with np.errstate(all="ignore"):                                            # (a c or f the library refuses gives nan or inf here)
        return np.sqrt(np.log(1.0 / wmin) / np.float64(c)) / (2.0 * np.pi * fa)


def wwz(y, t, f=None, tau=None, ntau=None, c=WWZ_DECAY, wmin=1e-9, W=None, center_data=True, coef=False, device=0):
    """Foster's weighted wavelet Z-transform (AJ 112, 1996) of non-uniformly sampled signals: at every time ``tau[j]`` and frequency
    ``f[k]`` the floating-mean fit ``y ≈ c + a cos 2πft + b sin 2πft`` of :func:`lombscargle` under the weights
    ``W exp(-c (2π f (t - tau))²)``, whose width is a fixed number of periods -- a time-frequency map whose resolution follows the
    frequency, where :func:`lombscargle_spectrogram` has one window length for all of them (csrc/wwz.hip; include/lpvspectral.h g8).

    ``y``: (N,) or (N, ns) signals sharing the non-decreasing times ``t`` (numpy arrays or device tensors); ``f``: positive frequencies
    (``None``: ``default_freqs(t)`` without its zero); ``tau``: the times, in any order (``None``: ``ntau`` -- default 64 -- equally spaced
    over ``[t[0], t[-1]]``); ``c``: the decay, Foster's ``1 / (8π²)`` (one period per sigma); ``wmin``: a sample whose weight would be
    below it is out of reach of a cell (:func:`wwz_radius`; ``1e-9`` is what Foster's own program uses, ``0`` makes every cell the whole
    record); ``W``: non-negative weights.  ``center_data`` removes the record's weighted mean first (numerics only: the fitted constant
    absorbs it).

    Returns a :class:`WWZ`; with ``coef=True`` also ``(a, b, c)`` (phase origin ``t = 0``; Foster's are these rotated by ``2π f tau``).
    Cells without samples (or with weights that underflow to 0) are exact zeros and flagged in ``empty``; ``Neff <= 3`` gives
    ``wwz = 0``; a fit exact to rounding gives ``wwz = inf``; nothing is ever NaN.  A column has the same bits whether its time is
    computed alone, among others or in another place of the list, and a signal the same bits alone and among others."""
    th = None
    if f is None or tau is None:
        th = np.ravel(_host(t))
    fa = np.ascontiguousarray(np.ravel(_host(default_freqs(th)[1:] if f is None else f)).astype(np.float64))
    if tau is None:
        n = 64 if ntau is None else int(ntau)
        if n < 1:
            raise ValueError(f"ntau must be at least 1, got {ntau!r}")
        ta = np.ascontiguousarray(np.linspace(th[0], th[-1], n))
    else:
        if ntau is not None:
            raise ValueError("give tau or ntau, not both")
        ta = np.ascontiguousarray(np.ravel(_host(tau)).astype(np.float64))
    Nf, Ntau = len(fa), len(ta)
    ra = np.ascontiguousarray(np.ravel(wwz_radius(fa, c, wmin)))
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    planes = np.zeros((3, ns, Ntau, Nf))                                       # power, amplitude, wwz: [signal][time][frequency]
    neff = np.zeros((Ntau, Nf))
    co = np.zeros((3, ns, Ntau, Nf)) if coef else None
    counts, empty = np.zeros((Ntau, Nf), dtype=np.int64), np.zeros((Ntau, Nf), dtype=np.int32)
    check(lib().lpvs_wwz_f64(py, ns, pt, N, pw, out_ptr(fa), Nf, out_ptr(ta), Ntau, float(c), out_ptr(ra), int(bool(center_data)), int(device),
                             out_ptr(planes[0]), out_ptr(planes[1]), out_ptr(planes[2]), out_ptr(neff), out_ptr(co) if coef else None,
                             out_ptr(counts), out_ptr(empty)))
    del ky, kt, kw

    def shaped(a):                                                             # (ns, Ntau, Nf) -> (Nf, Ntau) or (Nf, Ntau, ns)
        return np.ascontiguousarray(a[0].T) if single else np.ascontiguousarray(np.transpose(a, (2, 1, 0)))
    R = WWZ(shaped(planes[0]), fa, ta, shaped(planes[2]), shaped(planes[1]), np.ascontiguousarray(neff.T), np.ascontiguousarray(counts.T),
            np.ascontiguousarray(empty.T).astype(bool), ra)
    return (R, tuple(shaped(co[i]) for i in range(3))) if coef else R


def wwz_last_timing():
    """Plan and timing of the calling thread's last :func:`wwz`: the times and signals a thread of the sums kernel carries, the work items,
    the slab length, empty and degenerate cells, staged and useful (sample, frequency, time) triples, milliseconds per phase."""
    o = np.zeros(16)
    check(lib().lpvs_wwz_last_timing(out_ptr(o), 16))
    return {"nf": int(o[0]), "ntau": int(o[1]), "tt": int(o[2]), "ts": int(o[3]), "items": int(o[4]), "slab": int(o[5]), "empty": int(o[6]),
            "degenerate": int(o[7]), "staged": float(o[8]), "useful": float(o[9]), "scan_ms": float(o[10]), "ranges_ms": float(o[11]),
            "sums_ms": float(o[12]), "epilogue_ms": float(o[13]), "copy_ms": float(o[14]), "total_ms": float(o[15])}


# ---- box least squares periodogram (include/lpvspectral.h g9; csrc/bls.hip) ------------------------------------------------------------------
_BLS_NORMALIZATIONS = {"standard": 0, "chi2": 1}


class BLS:
    """The result of :func:`bls`.  ``freq``: (Nf,); ``power``, ``depth``, ``depth_err``, ``snr = depth / depth_err`` (0 where degenerate),
    ``start``, ``width`` (the best box's first bin and width in bins), ``q = width / nbins``, ``duration = q / f``,
    ``transit_time = (start + width / 2) / nbins / f`` (the box's centre, in units of ``t`` after a whole number of periods from
    ``t = 0``), ``count_in`` and ``degenerate``: (Nf,) or (Nf, ns).  With ``return_hist=True`` also ``hist`` -- the raw integer
    histograms, (Nf, 1 + ns, nbins) int64: row 0 the weights at the scale 2^-60 (the counts with ``W=None``), row 1 + c signal c -- and
    ``hcount`` (Nf, nbins), the samples per bin."""

    def __init__(self, freq, power, depth, depth_err, start, width, count_in, degenerate, nbins, hist=None, hcount=None):
        self.freq, self.power, self.depth, self.depth_err, self.start, self.width = freq, power, depth, depth_err, start, width
        self.count_in, self.degenerate, self.nbins, self.hist, self.hcount = count_in, degenerate, nbins, hist, hcount
        fcol = freq if power.ndim == 1 else freq[:, None]
        self.snr = np.divide(depth, depth_err, out=np.zeros_like(depth), where=depth_err > 0)
        self.q = width / float(nbins)
        self.duration = self.q / fcol
        self.transit_time = (start + width / 2.0) / float(nbins) / fcol


def bls_frequencies(t, fmin, fmax, qmin, oversample=3):
    """The frequency grid of a box search: from ``fmin`` up to ``fmax`` in steps of ``qmin / (oversample (max t - min t))`` -- over the
    record a box of the shortest relative duration ``qmin`` then drifts by ``1 / oversample`` of its width from one frequency to the
    next."""
    th = np.ravel(_host(t)).astype(np.float64)
    span = float(th.max() - th.min())
    if not (span > 0 and qmin > 0 and oversample > 0 and 0 < fmin <= fmax):
        raise ValueError(f"bls_frequencies: need max t > min t, qmin > 0, oversample > 0 and 0 < fmin <= fmax (span = {span}, qmin = {qmin}, "
                         f"oversample = {oversample}, fmin = {fmin}, fmax = {fmax})")
    df = qmin / (oversample * span)
    return fmin + df * np.arange(int(np.floor((fmax - fmin) / df)) + 1)


def bls(y, t, f, W=None, nbins=200, q=(0.01, 0.1), duration=None, min_count=1, dips_only=True, center_data=True, normalization="standard", device=0,
        return_hist=False):
    """Box least squares periodogram (Kovács, Zucker & Mazeh 2002, the binned form) of non-uniformly sampled signals: at every frequency
    the record is folded into ``nbins`` phase bins and every box of adjacent bins (wrapping) is tried as a two-level model.  It finds
    transits, eclipses and periodic drop-outs -- dips far shorter than a period, which no number of harmonics of
    :func:`lombscargle` describes (csrc/bls.hip; include/lpvspectral.h g9).

    ``y``: (N,) or (N, ns) signals sharing the times ``t`` (numpy arrays or device tensors; ``t`` in any order); ``f``: positive
    frequencies (:func:`bls_frequencies` makes the usual grid); ``W``: non-negative weights, inverse variances for ``depth_err``
    (``None``: ones).  The widths tried: ``q = (qmin, qmax)``, shares of a period, give ``kmin = max(1, floor(qmin nbins))`` and
    ``kmax = min(nbins // 2, ceil(qmax nbins))`` bins at every frequency; ``duration = (dmin, dmax)`` in units of ``t`` gives the same per
    frequency with ``q = d f``.  ``min_count``: the least number of samples inside and outside a box.  ``dips_only``: only boxes that
    lie below the rest.  ``normalization``: ``"standard"`` (the share of the weighted variance the box explains, in [0, 1]) or
    ``"chi2"`` (the fall of chi², ``snr²``).

    The folds use the phases of the exact products ``f t``; the sums -- the histograms and ``YY`` -- are 64-bit integer sums of the
    quantised record (csrc/bls_plan.h), so a frequency or a signal has the same bits whatever else is computed in the call, and with
    ``W=None, center_data=False`` a permutation of the samples changes no bit of any output (with weights or centring ``ΣW`` and the
    mean are floating-point tree sums in sample order, and a permutation may move the quantised record by a rounding).  Frequencies without a valid box, constant
    signals and samples that all fall in one bin give zeros, flagged in ``degenerate``; nothing is ever NaN.  Returns a :class:`BLS`."""
    if normalization not in _BLS_NORMALIZATIONS:
        raise ValueError(f"normalization: unknown value {normalization!r} (known: {sorted(_BLS_NORMALIZATIONS)})")
    fa = np.ascontiguousarray(np.ravel(_host(f)).astype(np.float64))
    Nf, nbins = len(fa), int(nbins)
    if duration is not None:
        qlo, qhi = float(duration[0]) * fa, float(duration[1]) * fa
    else:
        qlo, qhi = np.full(Nf, float(q[0])), np.full(Nf, float(q[1]))
    with np.errstate(all="ignore"):                                            # (a frequency the library refuses gives nan or inf here)
        kmin = np.nan_to_num(np.maximum(1.0, np.floor(qlo * nbins)), nan=0.0, posinf=2.0 ** 30, neginf=0.0)
        kmax = np.nan_to_num(np.minimum(float(nbins // 2), np.ceil(qhi * nbins)), nan=0.0, posinf=2.0 ** 30, neginf=0.0)
    kmin, kmax = np.ascontiguousarray(kmin.astype(np.int32)), np.ascontiguousarray(kmax.astype(np.int32))
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    planes = np.zeros((3, ns, Nf))                                             # power, depth, depth_err: [signal][frequency]
    ints = np.zeros((3, ns, Nf), dtype=np.int32)                               # start, width, degenerate
    count = np.zeros((ns, Nf), dtype=np.int64)
    hist = np.zeros((Nf, 1 + ns, max(nbins, 0)), dtype=np.int64) if return_hist else None
    hcount = np.zeros((Nf, max(nbins, 0)), dtype=np.int32) if return_hist else None
    check(lib().lpvs_bls_f64(py, ns, pt, N, pw, out_ptr(fa), Nf, nbins, out_ptr(kmin), out_ptr(kmax), int(min_count), int(bool(dips_only)),
                             int(bool(center_data)), _BLS_NORMALIZATIONS[normalization], int(device), out_ptr(planes[0]), out_ptr(planes[1]),
                             out_ptr(planes[2]), out_ptr(ints[0]), out_ptr(ints[1]), out_ptr(count), out_ptr(ints[2]),
                             out_ptr(hist) if return_hist else None, out_ptr(hcount) if return_hist else None))
    del ky, kt, kw

    def shaped(a):                                                             # (ns, Nf) -> (Nf,) or (Nf, ns)
        return a[0].copy() if single else np.ascontiguousarray(a.T)
    return BLS(fa, shaped(planes[0]), shaped(planes[1]), shaped(planes[2]), shaped(ints[0]), shaped(ints[1]), shaped(count), shaped(ints[2]).astype(bool),
               nbins, hist, hcount)


def bls_last_timing():
    """Plan and timing of the calling thread's last :func:`bls`: frequencies per workgroup, signals per pass, passes, LDS bytes, the
    shifts of the quantisation, degenerate (frequency, signal) pairs, boxes tried per signal, milliseconds per phase."""
    o = np.zeros(16)
    check(lib().lpvs_bls_last_timing(out_ptr(o), 16))
    return {"F": int(o[0]), "ts": int(o[1]), "passes": int(o[2]), "lds_bytes": int(o[3]), "shift_w": int(o[4]), "shift_y_min": int(o[5]),
            "shift_y_max": int(o[6]), "degenerate": int(o[7]), "boxes": float(o[8]), "unit": bool(o[9]), "scan_ms": float(o[10]),
            "quantise_ms": float(o[11]), "search_ms": float(o[12]), "copy_ms": float(o[13]), "total_ms": float(o[14]), "nf": int(o[15])}


# ---- fold statistics: pdm, aov, conditional_entropy (include/lpvspectral.h g10; csrc/fold.hip) ------------------------------------------------
class PDM:
    """The result of :func:`pdm` and :func:`aov`.  ``f``: (Nf,); ``theta`` (Stellingwerf's statistic: small at a period, 1 where
    degenerate), ``aov`` (the between / within F ratio: large at a period, 0 where degenerate, ``+inf`` where ``explained`` is 1; ``None``
    for ``covers > 1``), ``explained`` (the share of the weighted variance between the bins, pooled over the covers, in [0, 1]) and
    ``degenerate``: (Nf,) or (Nf, ns); ``nonempty``: (Nf,), the coarse bins that hold weight.  With ``return_hist=True`` also ``hist``
    -- the raw integer histograms over the ``nbins covers`` fine bins, (Nf, 1 + ns, nfine) int64, laid out as :class:`BLS`'s -- and
    ``hcount`` (Nf, nfine)."""

    def __init__(self, f, theta, aov, explained, nonempty, degenerate, nbins, covers, hist=None, hcount=None):
        self.f, self.theta, self.aov, self.explained, self.nonempty, self.degenerate = f, theta, aov, explained, nonempty, degenerate
        self.nbins, self.covers, self.hist, self.hcount = nbins, covers, hist, hcount


class CE:
    """The result of :func:`conditional_entropy`.  ``f``: (Nf,); ``entropy``: (Nf,) or (Nf, ns), in nats -- the period is at its
    MINIMUM; ``ylim``: (2,) or (ns, 2), the extremes the value bins span; ``degenerate``: a bool or (ns,), a constant signal (entropy 0);
    with ``return_hist=True`` ``hist``: the counts, (Nf, ns, nbins, mbins) int32."""

    def __init__(self, f, entropy, ylim, degenerate, nbins, mbins, hist=None):
        self.f, self.entropy, self.ylim, self.degenerate, self.nbins, self.mbins, self.hist = f, entropy, ylim, degenerate, nbins, mbins, hist


def pdm(y, t, f, W=None, nbins=10, covers=1, center_data=True, device=0, return_hist=False):
    """Phase dispersion minimisation (Stellingwerf 1978) of non-uniformly sampled signals, with his overlapping bin covers
    ``(Nb, Nc) = (nbins, covers)``: at every frequency the record is folded into ``nbins covers`` fine bins, a coarse bin is ``covers``
    adjacent fine bins (wrapping), and every one of the ``covers`` partitions into ``nbins`` bins is used.  It makes no assumption about
    the shape of the signal: sawtooth pulsators, binaries with unequal minima, repeating transients (csrc/fold.hip;
    include/lpvspectral.h g10).

    ``y``: (N,) or (N, ns) signals sharing the times ``t`` (numpy arrays or device tensors; ``t`` in any order); ``f``: positive
    frequencies; ``W``: non-negative weights (``None``: ones); ``2 <= nbins covers <= 2048``.  The device returns ``explained``, the
    share of the weighted variance that lies between the bins, pooled over the covers, and ``nonempty = M``, the coarse bins that hold
    weight; from them ``theta = (1 - explained) covers (N - 1) / (covers N - M)`` -- Stellingwerf's ``s² / σ²``, near 1 away from a
    period and small at one -- and, for ``covers = 1``, ``aov = explained / (1 - explained) (N - M) / (M - 1)``
    (Schwarzenberg-Czerny 1989).

    The fold uses the phases of the exact products ``f t`` and the sums are 64-bit integer sums of the quantised record
    (csrc/bls_plan.h, csrc/fold_plan.h): a frequency or a signal has the same bits whatever else is computed in the call, and with
    ``W=None, center_data=False`` a permutation of the samples changes no bit.  Constant signals, samples that all fall in one run of
    fine bins and folds that leave no degree of freedom give ``explained = 0, theta = 1, aov = 0``, flagged in ``degenerate``; nothing
    is ever NaN.  Returns a :class:`PDM`."""
    fa = np.ascontiguousarray(np.ravel(_host(f)).astype(np.float64))
    Nf, nbins, covers = len(fa), int(nbins), int(covers)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    nfine = nbins * covers if 0 < nbins <= 2048 and 0 < covers <= 2048 else 0
    explained = np.zeros((ns, Nf))
    nonempty = np.zeros(Nf, dtype=np.int32)
    degenerate = np.zeros((ns, Nf), dtype=np.int32)
    hist = np.zeros((Nf, 1 + ns, nfine), dtype=np.int64) if return_hist else None
    hcount = np.zeros((Nf, nfine), dtype=np.int32) if return_hist else None
    check(lib().lpvs_pdm_f64(py, ns, pt, N, pw, out_ptr(fa), Nf, nbins, covers, int(bool(center_data)), int(device), out_ptr(explained),
                             out_ptr(nonempty), out_ptr(degenerate), out_ptr(hist) if return_hist else None, out_ptr(hcount) if return_hist else None))
    del ky, kt, kw
    deg = degenerate != 0
    M = nonempty.astype(np.float64)[None, :]
    with np.errstate(all="ignore"):
        theta = np.where(deg, 1.0, (1.0 - explained) * (covers * (N - 1.0)) / (covers * float(N) - M))
        F = None
        if covers == 1:
            F = np.where(deg, 0.0, np.where(explained < 1.0, explained / (1.0 - explained) * (N - M) / (M - 1.0), np.inf))

    def shaped(a):                                                             # (ns, Nf) -> (Nf,) or (Nf, ns)
        return a[0].copy() if single else np.ascontiguousarray(a.T)
    return PDM(fa, shaped(theta), None if F is None else shaped(F), shaped(explained), nonempty, shaped(deg), nbins, covers, hist, hcount)


def aov(y, t, f, W=None, nbins=10, covers=1, center_data=True, device=0, return_hist=False):
    """The analysis-of-variance periodogram (Schwarzenberg-Czerny 1989): :func:`pdm` with one cover, whose ``aov`` is the F ratio of the
    variance between the phase bins to the variance within them.  ``covers`` other than 1 is refused.  Returns a :class:`PDM`."""
    if int(covers) != 1:
        raise ValueError(f"aov: covers must be 1, got {covers}")
    return pdm(y, t, f, W=W, nbins=nbins, covers=1, center_data=center_data, device=device, return_hist=return_hist)


def pdm_last_timing():
    """Plan and timing of the calling thread's last :func:`pdm` or :func:`aov`."""
    o = np.zeros(16)
    check(lib().lpvs_pdm_last_timing(out_ptr(o), 16))
    return _fold_timing(o)


def _fold_timing(o):
    return {"F": int(o[0]), "ts": int(o[1]), "passes": int(o[2]), "lds_bytes": int(o[3]), "copies": int(o[4]), "shift_w": int(o[5]),
            "shift_y_min": int(o[6]), "shift_y_max": int(o[7]), "degenerate": int(o[8]), "unit": bool(o[9]), "scan_ms": float(o[10]),
            "prepare_ms": float(o[11]), "fold_ms": float(o[12]), "copy_ms": float(o[13]), "total_ms": float(o[14]), "nf": int(o[15])}


def conditional_entropy(y, t, f, nbins=10, mbins=5, device=0, return_hist=False):
    """The conditional-entropy periodogram (Graham et al. 2013) of non-uniformly sampled signals: at every frequency the samples are
    counted in ``nbins`` phase bins times ``mbins`` value bins (the values scaled to ``[min y, max y]`` per signal), and
    ``H = Σ p_ij ln(p_i / p_ij)`` is the Shannon entropy of the value bin given the phase bin, in nats.  A fold at the period
    orders the samples and LOWERS it: the period is at the minimum.  It is unweighted by definition (csrc/fold.hip;
    include/lpvspectral.h g10).  ``2 <= nbins <= 256``, ``2 <= mbins <= 64``, ``nbins mbins <= 8192``.

    Every sum is an integer count: a permutation of the samples changes no bit of any output, and a frequency or a signal has the same
    bits whatever else is computed in the call.  A constant signal has entropy 0 and is flagged in ``degenerate``.  Returns a
    :class:`CE`."""
    fa = np.ascontiguousarray(np.ravel(_host(f)).astype(np.float64))
    Nf, nbins, mbins = len(fa), int(nbins), int(mbins)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    cells = nbins * mbins if 0 < nbins <= 256 and 0 < mbins <= 64 else 0
    entropy = np.zeros((ns, Nf))
    ylim = np.zeros((ns, 2))
    degenerate = np.zeros(ns, dtype=np.int32)
    hist = np.zeros((Nf, ns, nbins, mbins) if cells else (0,), dtype=np.int32) if return_hist else None
    check(lib().lpvs_cent_f64(py, ns, pt, N, out_ptr(fa), Nf, nbins, mbins, int(device), out_ptr(entropy), out_ptr(ylim), out_ptr(degenerate),
                              out_ptr(hist) if return_hist else None))
    del ky, kt
    deg = degenerate != 0
    if single:
        return CE(fa, entropy[0].copy(), ylim[0].copy(), bool(deg[0]), nbins, mbins, hist)
    return CE(fa, np.ascontiguousarray(entropy.T), ylim, deg, nbins, mbins, hist)


def cent_last_timing():
    """Plan and timing of the calling thread's last :func:`conditional_entropy`; ``copies``: the private copies of the count histogram."""
    o = np.zeros(16)
    check(lib().lpvs_cent_last_timing(out_ptr(o), 16))
    return _fold_timing(o)


# ---- CLEAN deconvolution of the spectra of unevenly sampled records (include/lpvspectral.h g11; csrc/clean.hip) -------------------------------
_CLEAN_STATUS = {0: "niter", 1: "tol", 2: "empty"}
_CLEAN_HWHM_TO_SIGMA = 0.8493218002880191          # 1 / sqrt(2 ln 2)


class CLEAN:
    """The result of :func:`clean`.  With K = Nf - 1 and one signal (several: a leading or trailing ``ns`` as noted): ``freq`` (Nf,), the
    grid ``m df``; ``dirty`` (Nf,) or (Nf, ns) complex, the dirty spectrum ``D``; ``window`` (2 Nf - 1,) complex, the spectral window
    ``Wn``; ``residual`` and ``components``: ``R`` and ``C``, shaped as ``dirty``; ``picks`` (niter,) or (ns, niter) int32, the bins in
    the order picked, -1 behind the last, and ``pick_values``, the complex ``c`` of each pick; ``spectrum``: the restored ``S``,
    ``power = |S|²`` and ``amplitude = 2 |C|`` (the amplitude of the sinusoid a component stands for), shaped as ``dirty``;
    ``iterations`` and ``status`` (``"niter"``, ``"tol"`` or ``"empty"``): an int and a string, or (ns,) arrays / lists; ``sigma``: the
    width of the restoring beam, in the unit of ``freq``."""

    def __init__(self, freq, dirty, window, residual, components, picks, pick_values, spectrum, iterations, status, sigma):
        self.freq, self.dirty, self.window, self.residual, self.components = freq, dirty, window, residual, components
        self.picks, self.pick_values, self.spectrum, self.iterations, self.status, self.sigma = picks, pick_values, spectrum, iterations, status, sigma
        self.power = spectrum.real ** 2 + spectrum.imag ** 2
        self.amplitude = 2.0 * np.abs(components)


def _clean_grid(t, df, Nf):
    """``(df, Nf)`` with the defaults ``df = 1 / (4 (max t - min t))`` and ``Nf`` the grid up to ``default_freqs(t)``'s top frequency."""
    if df is None or Nf is None:
        th = _host(t)
        if df is None:
            span = float(np.max(th) - np.min(th))
            if not span > 0:
                raise ValueError("clean: df=None needs a record that spans more than one instant")
            df = 1.0 / (4.0 * span)
        if Nf is None:
            Nf = max(2, int(np.floor(float(default_freqs(th)[-1]) / float(df))) + 1)
    return float(df), int(Nf)


def _clean_complex(a, shape, what):
    """A host complex array or a device complex tensor as what the library reads: (keepalive, pointer), interleaved (re, im) doubles."""
    if _lib.is_device_array(a):
        import torch
        if a.dtype != torch.complex128 or tuple(a.shape) != tuple(shape):
            raise ValueError(f"{what}: a complex128 tensor of shape {tuple(shape)} is needed")
        r = torch.view_as_real(a.contiguous())
        torch.cuda.current_stream(r.device).synchronize()
        return r, C.c_void_p(r.data_ptr())
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.complex128))
    if arr.shape != tuple(shape):
        raise ValueError(f"{what}: shape {arr.shape}, needed {tuple(shape)}")
    return arr, out_ptr(arr)


def clean_sigma(Wn, df):
    """The width of the Gaussian restoring beam fitted to the spectral window ``Wn`` (2 Nf - 1 complex values on the grid ``m df``):
    the first ``m`` with ``|Wn_m|² < 1/2`` -- the half-power point of the main lobe --, interpolated linearly in ``|Wn|²``, is the half
    width ``h``; ``sigma = h / sqrt(2 ln 2)``.  The same operations, in the same order, as csrc/clean_plan.h ``clean_sigma``."""
    Wn = np.asarray(Wn, dtype=np.complex128)
    P = Wn.real * Wn.real + Wn.imag * Wn.imag
    df = np.float64(df)
    for m in range(1, len(P)):
        if P[m] < 0.5:
            prev = P[m - 1]
            frac = (prev - 0.5) / (prev - P[m]) if prev > P[m] else np.float64(0.0)
            return float(((np.float64(m - 1) + frac) * df) * np.float64(_CLEAN_HWHM_TO_SIGMA))
    return float((np.float64(len(P) - 1) * df) * np.float64(_CLEAN_HWHM_TO_SIGMA))


def dirty_spectrum(y, t, df=None, Nf=None, W=None, center_data=True, path="auto", device=0):
    """The dirty spectrum and the spectral window of non-uniformly sampled signals on the grid ``f_m = m df``:
    ``D_k = Σ w y_c e^{-2πi f_k t}`` for ``k = 0 .. Nf - 1`` and ``Wn_m = Σ w e^{-2πi f_m t}`` for ``m = 0 .. 2 Nf - 2`` -- the sums
    ``YC - i YS`` and ``C - i S`` of :func:`lombscargle`, by the same kernels and paths, with the weights normalised to sum 1 and the
    weighted mean removed (``center_data``).  ``y``: (N,) or (N, ns); defaults: ``df = 1 / (4 (max t - min t))``, ``Nf`` up to
    ``default_freqs(t)``'s top frequency.  Returns ``(D, Wn)``: complex arrays of shape (Nf,) or (ns, Nf), and (2 Nf - 1,)."""
    if path not in _EVAL_PATHS:
        raise ValueError(f"path: unknown value {path!r} (known: {sorted(_EVAL_PATHS)})")
    df, Nf = _clean_grid(t, df, Nf)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    D = np.zeros((ns, max(Nf, 0)), dtype=np.complex128)
    Wn = np.zeros(max(2 * Nf - 1, 0), dtype=np.complex128)
    check(lib().lpvs_dirty_spectrum_f64(py, ns, pt, N, pw, df, Nf, int(bool(center_data)), _EVAL_PATHS[path], int(device), out_ptr(D), out_ptr(Wn)))
    del ky, kt, kw
    return (D[0].copy() if single else D), Wn


def clean_loop(D, Wn, gain=0.5, niter=100, tol=0.0, device=0):
    """The CLEAN loop (Roberts, Lehár & Dreher 1987) on spectra the caller has: ``D`` (Nf,) or (ns, Nf) complex, ``Wn`` (2 Nf - 1,)
    complex (numpy arrays or complex128 device tensors).  Per iteration: the admissible bin ``p`` of the largest ``|R|²`` (admissible:
    ``1 - |Wn_2p|² >= 2^-20``; ties to the lowest index), ``a = (R_p - conj(R_p) Wn_2p) / (1 - |Wn_2p|²)``, ``c = gain a``,
    ``C_p += c`` and ``R_k -= c Wn_{k-p} + conj(c) Wn_{k+p}`` for every ``k`` -- all iterations of a signal in ONE kernel launch, the
    residual resident in LDS (csrc/clean.hip).  It stops after ``niter`` picks, when the peak has fallen to ``tol`` times the first
    peak's modulus (``tol = 0``: never) or when no bin is admissible.  ``gain`` in (0, 2).

    Returns ``(R, C, picks, pick_values, iterations, status)``: ``R``, ``C`` shaped as ``D``; ``picks`` (niter,) or (ns, niter) int32
    (-1 behind the last pick) and the complex ``pick_values``; ``iterations`` and ``status`` (0 niter, 1 tol, 2 empty): ints, or (ns,)
    int32 arrays.  Every operation is a rounded double operation in the order include/lpvspectral.h g11 states: the result does not
    depend on the thread count or on where the residual lives."""
    D = D if _lib.is_device_array(D) else np.asarray(D, dtype=np.complex128)
    single = len(D.shape) == 1
    shape = tuple(D.shape) if not single else (1, int(D.shape[0]))
    ns, Nf = int(shape[0]), int(shape[1])
    kD, pD = _clean_complex(D.reshape(shape) if single else D, shape, "D")
    kW, pW = _clean_complex(Wn, (2 * Nf - 1,), "Wn")
    niter = int(niter)
    nit = max(niter, 0)
    R = np.zeros((ns, Nf), dtype=np.complex128)
    Cc = np.zeros((ns, Nf), dtype=np.complex128)
    picks = np.full((ns, nit), -1, dtype=np.int32)
    pv = np.zeros((ns, nit), dtype=np.complex128)
    iters = np.zeros(ns, dtype=np.int32)
    status = np.zeros(ns, dtype=np.int32)
    spare = np.zeros(2)                                                       # (pointers of empty arrays are not NULL to the library)
    check(lib().lpvs_clean_loop_f64(pD, ns, Nf, pW, float(gain), niter, float(tol), int(device), out_ptr(R), out_ptr(Cc),
                                    out_ptr(picks) if nit else out_ptr(spare), out_ptr(pv) if nit else out_ptr(spare), out_ptr(iters), out_ptr(status)))
    del kD, kW
    if single:
        return R[0], Cc[0], picks[0], pv[0], int(iters[0]), int(status[0])
    return R, Cc, picks, pv, iters, status


def clean_restore(R, C_, df, sigma, device=0):
    """The restored spectrum ``S_k = R_k + Σ_p [C_p B_{k-p} + conj(C_p) B_{k+p}]`` with the real Gaussian beam
    ``B_m = exp(-(m df)² / (2 sigma²))``, summed over the nonzero components in increasing ``p`` by a gather on the device.  ``R``,
    ``C_``: (Nf,) or (ns, Nf) complex.  Returns ``S`` shaped as ``R``."""
    R = R if _lib.is_device_array(R) else np.asarray(R, dtype=np.complex128)
    C_ = C_ if _lib.is_device_array(C_) else np.asarray(C_, dtype=np.complex128)
    single = len(R.shape) == 1
    shape = tuple(R.shape) if not single else (1, int(R.shape[0]))
    ns, Nf = int(shape[0]), int(shape[1])
    kR, pR = _clean_complex(R.reshape(shape) if single else R, shape, "R")
    kC, pC = _clean_complex(C_.reshape(shape) if single else C_, shape, "C")
    S = np.zeros((ns, Nf), dtype=np.complex128)
    check(lib().lpvs_clean_restore_f64(pR, pC, ns, Nf, float(df), float(sigma), int(device), out_ptr(S)))
    del kR, kC
    return S[0] if single else S


def clean(y, t, df=None, Nf=None, W=None, gain=0.5, niter=100, tol=0.0, center_data=True, center_time=True, path="auto", device=0):
    """CLEAN deconvolution (Roberts, Lehár & Dreher 1987) of the spectrum of non-uniformly sampled signals: :func:`dirty_spectrum`,
    :func:`clean_loop` and :func:`clean_restore` in one call of the library, the spectra staying on the device between the stages.
    Uneven sampling convolves every line of a spectrum with the spectral window -- one sinusoid shows as a forest of sidelobes and
    aliases --; CLEAN removes the window's response to the strongest line, ``gain`` of it at a time, and leaves a short list of
    complex ``components`` (``amplitude = 2 |C|`` and ``angle(C)`` are the amplitude and the phase of a sinusoid) and a ``residual``.
    The restored ``spectrum`` puts the components back under a Gaussian beam as wide as the window's main lobe.

    ``y``: (N,) or (N, ns) signals sharing the times ``t``; ``W``: non-negative weights (``None``: ones).  ``df``, ``Nf``: the grid
    ``m df``, ``m = 0 .. Nf - 1`` (the window is formed up to ``2 (Nf - 1) df``); defaults ``df = 1 / (4 (max t - min t))`` and
    ``Nf`` up to ``default_freqs(t)``'s top frequency.  ``center_time=True`` subtracts ``np.mean(t)`` on the host first: the beam is
    real, so phases refer to the mean epoch, as in the paper.  This redefines the record by one rounding per time; pass
    ``center_time=False`` for the bits of the record as given (phases then refer to ``t = 0``).  Returns a :class:`CLEAN`.

    Not covered: one signal is one workgroup (a lone signal runs on one compute unit: the loop is bound by latency), beams other than
    the Gaussian, and several harmonics per component."""
    if path not in _EVAL_PATHS:
        raise ValueError(f"path: unknown value {path!r} (known: {sorted(_EVAL_PATHS)})")
    df, Nf = _clean_grid(t, df, Nf)
    if center_time:
        th = _host(t)
        t = th - np.mean(th)
    ys, N, ns, single = _lomb_signals(y)
    ky, py, ny = as_f64(ys)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    niter = int(niter)
    nit, nf = max(niter, 0), max(Nf, 0)
    D, R, Cc, S = (np.zeros((ns, nf), dtype=np.complex128) for _ in range(4))
    Wn = np.zeros(max(2 * Nf - 1, 0), dtype=np.complex128)
    picks = np.full((ns, nit), -1, dtype=np.int32)
    pv = np.zeros((ns, nit), dtype=np.complex128)
    iters = np.zeros(ns, dtype=np.int32)
    status = np.zeros(ns, dtype=np.int32)
    sigma = C.c_double(0.0)
    spare = np.zeros(2)
    check(lib().lpvs_clean_f64(py, ns, pt, N, pw, df, Nf, int(bool(center_data)), _EVAL_PATHS[path], float(gain), niter, float(tol), 0.0, int(device),
                               out_ptr(D), out_ptr(Wn), out_ptr(R), out_ptr(Cc), out_ptr(picks) if nit else out_ptr(spare),
                               out_ptr(pv) if nit else out_ptr(spare), out_ptr(iters), out_ptr(status), out_ptr(S), C.byref(sigma)))
    del ky, kt, kw
    freq = np.arange(Nf) * df
    if single:
        return CLEAN(freq, D[0], Wn, R[0], Cc[0], picks[0], pv[0], S[0], int(iters[0]), _CLEAN_STATUS[int(status[0])], float(sigma.value))
    shaped = lambda a: np.ascontiguousarray(a.T)                               # noqa: E731  (ns, Nf) -> (Nf, ns)
    return CLEAN(freq, shaped(D), Wn, shaped(R), shaped(Cc), picks, pv, shaped(S), iters, [_CLEAN_STATUS[int(v)] for v in status], float(sigma.value))


def clean_last_timing():
    """Plan and timing of the calling thread's last :func:`dirty_spectrum`, :func:`clean_loop`, :func:`clean_restore` or :func:`clean`
    (0 / ``"none"`` where the call had no such stage): the path of the sums, where the residual lived, the threads and the LDS bytes
    of the loop's workgroup, the fewest and the most iterations of a signal, the admissible bins, milliseconds per stage."""
    o = np.zeros(14)
    check(lib().lpvs_clean_last_timing(out_ptr(o), 14))
    return {"path": {1: "direct", 2: "nufft"}.get(int(o[0]), "none"), "residual": {1: "lds", 2: "global"}.get(int(o[1]), "none"), "threads": int(o[2]),
            "lds_bytes": int(o[3]), "iterations_min": int(o[4]), "iterations_max": int(o[5]), "admissible": int(o[6]), "moments_ms": float(o[7]),
            "sums_ms": float(o[8]), "loop_ms": float(o[9]), "restore_ms": float(o[10]), "copy_ms": float(o[11]), "total_ms": float(o[12]),
            "sigma": float(o[13])}


# ---- false-alarm probabilities of the Lomb-Scargle periodogram: the device bootstrap and the closed forms (include/lpvspectral.h g6) ------
_M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of uint64 that hold 32-bit words (csrc/philox.h)."""
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _mulhi64(u, n):
    """High 64 bits of the product of the uint64 arrays u and the integer n < 2^64 (32-bit limbs in uint64 arithmetic)."""
    s32 = np.uint64(32)
    nl, nh = np.uint64(n & 0xFFFFFFFF), np.uint64(n >> 32)
    ul, uh = u & _M32, u >> s32
    t1 = uh * nl + ((ul * nl) >> s32)
    t2 = ul * nh + (t1 & _M32)
    return uh * nh + (t1 >> s32) + (t2 >> s32)


def bootstrap_indices(N, B, seed=0, row0=0, samples=None):
    """The resampling indices of :func:`lombscargle_bootstrap` on the host: ``int64[B, N]``, row ``b`` holding ``π_{row0+b}(i)``, so that
    resample ``row0 + b`` of a record ``y`` is ``y[indices[b]]``.

    The stream: Philox4x32-10 as :func:`randn` keys it -- key = the 64-bit ``seed``, counter = (resample, pair ``i >> 1``), words
    ``w0..w3``; sample ``2p`` takes ``u = (w0 << 32) | w1``, sample ``2p+1`` takes ``u = (w2 << 32) | w3``; ``π = (u N) >> 64``.  Every
    index lies in ``[0, N)``; a resample depends on ``(seed, row0 + b)`` only.  ``samples``: only these sample positions ``i`` (columns),
    for records too long to list."""
    N, B, row0 = int(N), int(B), int(row0)
    if N < 1 or B < 1 or row0 < 0 or N >= 1 << 63:
        raise ValueError(f"bootstrap_indices: need N > 0, B > 0 and row0 >= 0 (N = {N}, B = {B}, row0 = {row0})")
    i = np.arange(N, dtype=np.uint64) if samples is None else np.ravel(np.asarray(samples)).astype(np.uint64)
    if len(i) and int(i.max()) >= N:
        raise ValueError("bootstrap_indices: samples reach beyond N")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    b = (np.arange(B, dtype=np.uint64) + np.uint64(row0))[:, None]
    p = (i >> np.uint64(1))[None, :]
    b, p = np.broadcast_arrays(b, p)
    w0, w1, w2, w3 = _philox4x32_10(b & _M32, b >> np.uint64(32), p & _M32, p >> np.uint64(32), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    odd = (i & np.uint64(1)).astype(bool)[None, :]
    u = np.where(odd, (w2 << np.uint64(32)) | w3, (w0 << np.uint64(32)) | w1)
    return _mulhi64(u, N).astype(np.int64)


def lombscargle_bootstrap(y, t, f=None, W=None, B=1000, seed=0, row0=0, fit_mean=True, center_data=True, normalization="standard", device=0,
                          return_argmax=False, return_means=False, return_power=False):
    """The maxima of the :func:`lombscargle` periodograms of ``B`` resamples of one record, on the device (extension; csrc/lomb_boot.hip):
    what :func:`false_alarm_probability` and :func:`false_alarm_level` with ``method="bootstrap"`` are read from.

    Resample ``b`` is ``y[π_b]`` (:func:`bootstrap_indices`, resamples ``row0 .. row0 + B - 1`` of ``seed``); ``t`` and ``W`` stay with
    the epochs (astropy resamples ``(y, dy)`` pairs instead).  Each resample's periodogram is the :func:`lombscargle` estimate with the
    same flags; only its maximum leaves the device: neither the resamples nor the ``B × Nf`` powers are ever stored.  Two calls give the
    same bits, and a resample's result does not depend on ``B``, ``row0`` or the other resamples.

    Returns the maxima ``(B,)``; with ``return_argmax`` / ``return_means`` / ``return_power`` a tuple that adds the frequency index of
    each maximum (ties: the lowest), the weighted mean of each resample as the device formed it, and the columns ``(Nf, B)``."""
    if normalization not in _LOMB_NORMALIZATIONS:
        raise ValueError(f"normalization: unknown value {normalization!r} (known: {sorted(_LOMB_NORMALIZATIONS)})")
    fa = np.ascontiguousarray(np.ravel(_host(default_freqs(t) if f is None else f)).astype(np.float64))
    Nf, B = len(fa), int(B)
    ya = _f64_arg(y)
    if (ya.dim() if _lib.is_device_array(ya) else np.ndim(ya)) != 1:
        raise ValueError("lombscargle_bootstrap: y is one signal (a vector)")
    ky, py, N = as_f64(ya)
    kt, pt, nt = as_f64(_f64_arg(t))
    if nt != N:
        raise ValueError(f"y has {N} samples, t has {nt}")
    kw, pw, nw = as_f64(_f64_arg(W))
    if W is not None and nw != N:
        raise ValueError(f"y has {N} samples, W has {nw}")
    nb = max(B, 1)
    maxima, argmax, means = np.zeros(nb), np.zeros(nb, dtype=np.int64), np.zeros(nb)
    power = np.zeros((Nf, nb), order="F") if return_power else None
    check(lib().lpvs_lombscargle_bootstrap_f64(py, pt, N, pw, out_ptr(fa), Nf, B, int(seed), int(row0), int(bool(fit_mean)), int(bool(center_data)),
                                               _LOMB_NORMALIZATIONS[normalization], int(device), out_ptr(maxima), out_ptr(argmax), out_ptr(means),
                                               out_ptr(power) if return_power else None))
    del ky, kt, kw
    res = [maxima] + ([argmax] if return_argmax else []) + ([means] if return_means else []) + ([power] if return_power else [])
    return res[0] if len(res) == 1 else tuple(res)


def lombscargle_bootstrap_last_timing():
    """Plan and timing of the calling thread's last :func:`lombscargle_bootstrap`."""
    o = np.zeros(12)
    check(lib().lpvs_lombscargle_bootstrap_last_timing(out_ptr(o), 12))
    return {"resamples": int(o[0]), "chunks": int(o[1]), "ts": int(o[2]), "slab": int(o[3]), "slabs": int(o[4]), "degenerate": int(o[5]),
            "shared_ms": float(o[6]), "moments_ms": float(o[7]), "sums_ms": float(o[8]), "epilogue_ms": float(o[9]), "copy_ms": float(o[10]),
            "total_ms": float(o[11])}


_FAP_METHODS = ("naive", "davies", "baluev", "bootstrap")
_LDF = np.longdouble


def _fap_setup(y, t, f, W, fit_mean, center_data, normalization, method):
    """(N_H, N_K, f_max T, gamma(N_H) f_max sqrt(4 pi Var_w t)) of the analytic methods, as long doubles."""
    import math
    if normalization != "standard":
        raise ValueError(f"method {method!r} is defined for normalization='standard' only (the null distribution of 'psd' needs the noise variance); "
                         "use method='bootstrap'")
    th = np.ravel(_host(t)).astype(np.float64)
    N = len(th)
    fa = np.ravel(_host(default_freqs(t) if f is None else f)).astype(np.float64)
    NH = N - (1 if (fit_mean or center_data) else 0)
    NK = NH - 2
    if NK < 2:
        raise ValueError(f"false alarm: {N} samples are too few")
    fmax = _LDF(fa.max())
    tl = th.astype(_LDF)
    w = np.ones(N, dtype=_LDF) if W is None else np.ravel(_host(W)).astype(np.float64).astype(_LDF)
    w = w / w.sum()
    var = (w * tl * tl).sum() - (w * tl).sum() ** 2
    gam = np.sqrt(_LDF(2) / NH) * np.exp(_LDF(math.lgamma(NH / 2) - math.lgamma((NH - 1) / 2)))
    pi = np.arccos(_LDF(-1))
    return NH, NK, fmax * (tl.max() - tl.min()), gam * fmax * np.sqrt(4 * pi * var)


def _fap_analytic(z, method, NH, NK, neff, tau0):
    """The false-alarm probability of the peak heights z (long doubles) by one of the closed forms."""
    one = _LDF(1)
    lz = np.log1p(-z)                                                         # log(1 - z)
    single = np.exp(_LDF(NK) / 2 * lz)
    if method == "naive":
        return -np.expm1(neff * np.log1p(-single))
    tau = tau0 * np.exp(_LDF(NK - 1) / 2 * lz) * np.sqrt(_LDF(NH) * z / 2)
    if method == "davies":
        return single + tau
    return -np.expm1(np.log1p(-single) - tau)                                 # baluev: 1 - (1 - single) exp(-tau)


def _bootstrap_maxima(y, t, f, W, fit_mean, center_data, normalization, B, seed, maxima, device):
    if maxima is not None:
        M = np.ravel(np.asarray(maxima, dtype=np.float64))
        if len(M) < 1:
            raise ValueError("maxima: empty")
        return M
    return lombscargle_bootstrap(y, t, f, W=W, B=B, seed=seed, fit_mean=fit_mean, center_data=center_data, normalization=normalization, device=device)


def false_alarm_probability(power, y, t, f=None, W=None, method="baluev", fit_mean=True, center_data=True, normalization="standard", B=1000, seed=0,
                            maxima=None, device=0):
    """The probability that noise alone gives a highest periodogram peak of at least ``power`` (a scalar or an array; the result has its
    shape) for the record ``y, t, W`` and the grid ``f`` of :func:`lombscargle`.

    ``method``: ``"naive"``, ``"davies"``, ``"baluev"`` -- closed forms for ``normalization="standard"`` (ValueError for ``"psd"``), with
    ``N_H = N - d_H`` (``d_H = 1`` if ``fit_mean or center_data``), ``N_K = N_H - 2``, ``single = (1 - z)^(N_K/2)``, ``T = max t - min t``,
    ``τ = γ(N_H) f_max √(4π Var_w t) (1 - z)^((N_K-1)/2) √(N_H z / 2)``, ``γ(n) = √(2/n) exp(lgamma(n/2) - lgamma((n-1)/2))``:
    ``naive = 1 - (1 - single)^(f_max T)``, ``davies = single + τ``, ``baluev = 1 - (1 - single) e^{-τ}`` -- or ``"bootstrap"``: the
    distribution-free estimate ``#{M_b ≥ z} / B`` from the maxima ``M_b`` of ``B`` resampled periodograms (:func:`lombscargle_bootstrap`,
    with ``seed`` and the estimator's flags, either normalisation); ``maxima``: the maxima of an earlier call, to reuse them."""
    if method not in _FAP_METHODS:
        raise ValueError(f"method: unknown value {method!r} (known: {list(_FAP_METHODS)})")
    z = np.asarray(power, dtype=np.float64)
    if method == "bootstrap":
        M = np.sort(_bootstrap_maxima(y, t, f, W, fit_mean, center_data, normalization, B, seed, maxima, device))
        res = (len(M) - np.searchsorted(M, z, side="left")) / len(M)           # #{M >= z} / B
    else:
        NH, NK, neff, tau0 = _fap_setup(y, t, f, W, fit_mean, center_data, normalization, method)
        res = np.asarray(_fap_analytic(z.astype(_LDF), method, NH, NK, neff, tau0), dtype=np.float64)
    return float(res) if np.ndim(power) == 0 else res


def false_alarm_level(probability, y, t, f=None, W=None, method="baluev", fit_mean=True, center_data=True, normalization="standard", B=1000, seed=0,
                      maxima=None, device=0):
    """The peak height whose :func:`false_alarm_probability` is ``probability`` (a scalar or an array), by the same ``method``.

    ``"naive"`` is inverted in closed form; ``"davies"`` and ``"baluev"`` by bisection on ``[1/N_K, 1)``, where both decrease (``τ`` peaks
    at ``z = 1/N_K``), until the bracket no longer shrinks -- a probability above the value at ``1/N_K`` raises ValueError;
    ``"bootstrap"``: the order statistic ``M_(k)``, the k-th smallest maximum with ``k = clamp(ceil((1 - p) B), 1, B)``, no interpolation."""
    import math
    if method not in _FAP_METHODS:
        raise ValueError(f"method: unknown value {method!r} (known: {list(_FAP_METHODS)})")
    p = np.asarray(probability, dtype=np.float64)
    if np.any(~(p > 0)) or np.any(~(p <= 1)):
        raise ValueError("probability: values in (0, 1] are needed")
    flat = np.ravel(p)
    if method == "bootstrap":
        M = np.sort(_bootstrap_maxima(y, t, f, W, fit_mean, center_data, normalization, B, seed, maxima, device))
        nb = len(M)
        out = np.array([M[min(max(math.ceil((1.0 - float(q)) * nb), 1), nb) - 1] for q in flat])
    else:
        NH, NK, neff, tau0 = _fap_setup(y, t, f, W, fit_mean, center_data, normalization, method)
        out = np.zeros(len(flat))
        for i, q in enumerate(flat):
            ql = _LDF(q)
            if method == "naive":
                single = -np.expm1(np.log1p(-ql) / neff) if q < 1 else _LDF(1)
                out[i] = float(-np.expm1(np.log(single) * 2 / _LDF(NK)))
                continue
            lo, hi = _LDF(1) / NK, _LDF(1)
            if _fap_analytic(lo, method, NH, NK, neff, tau0) < ql:
                raise ValueError(f"probability {q} is above the {method} value at z = 1/N_K, beyond which the bound does not decrease")
            while True:                                                        # fap(lo) >= q > fap(hi)
                mid = lo + (hi - lo) / 2
                if not (lo < mid < hi):
                    break
                if _fap_analytic(mid, method, NH, NK, neff, tau0) >= ql:
                    lo = mid
                else:
                    hi = mid
            out[i] = float(lo)
    return float(out[0]) if np.ndim(probability) == 0 else out.reshape(p.shape)


def compress_last_timing():
    """Plan and HIP-event times (ms) of this thread's last compress / heatmap call."""
    o = np.zeros(5)
    check(lib().lpvs_compress_last_timing(out_ptr(o), 5))
    return dict(passes=int(o[0]), select_ms=o[1], clamp_ms=o[2], total_ms=o[3], digits_skipped=int(o[4]))


# --------------------------------------------------------------------------- ComplexNormal, the SpectralExt recipe's numbers, detrend
# (src/utilities.jl:1-17, :80-174, src/plotting.jl:54-106; csrc/cnormal.hip)
def _herm_upper(A):
    """``Hermitian(A)`` / ``Symmetric(A)`` for real A: the upper triangle decides (Julia's default ``:U``)."""
    A = np.asarray(A)
    U = np.triu(A, 1)
    return U + U.conj().T + np.diag(np.diag(A).real)


def _sym_upper(A):
    """``Symmetric(A)`` (no conjugation, also for complex A)."""
    A = np.asarray(A)
    return np.triu(A) + np.triu(A, 1).T


def _chol_upper(A):
    """``cholesky(A).U`` of a small dense host matrix: U'U = A (numpy's factor is the lower one)."""
    try:
        return np.linalg.cholesky(_herm_upper(A)).conj().T
    except np.linalg.LinAlgError as e:
        raise _lib.NumericError(f"matrix is not positive definite (PosDefException): {e}") from None


def _gamma_c(a, C=None):
    """(Γ, C) of a call ``f(Γ, C)`` or ``f(cn)`` (src/utilities.jl:141-143)."""
    if isinstance(a, ComplexNormal):
        return a.Γ, a.C
    return np.asarray(a), np.asarray(C)


def cn_V2ΓC(V):
    """src/utilities.jl:113-124 -> ``(Γ, C)`` as matrices.  The reference factors Γ here; this mirror keeps the matrix and factors it
    when :func:`pdf` asks (an 8192 × 8192 Σ costs nothing until then), so ``Matrix(Γ)`` is Γ itself, not the product of its rounded factors."""
    V = _sym_upper(np.asarray(V, dtype=np.float64))
    n = V.shape[0] // 2
    Vxx, Vyy, Vxy, Vyx = V[:n, :n], V[n:, n:], V[:n, n:], V[n:, :n]
    return (Vxx + Vyy) + 1j * (Vyx - Vxy), _sym_upper((Vxx - Vyy) + 1j * (Vyx + Vxy))


def cn_fVxx(Γ, C=None):
    Γ, C = _gamma_c(Γ, C)
    return (Γ + C).real / 2          # src/utilities.jl:131


def cn_fVyy(Γ, C=None):
    Γ, C = _gamma_c(Γ, C)
    return (Γ - C).real / 2          # :132


def cn_fVxy(Γ, C=None):
    Γ, C = _gamma_c(Γ, C)
    return (-Γ + C).imag / 2         # :133


def cn_fVyx(Γ, C=None):
    Γ, C = _gamma_c(Γ, C)
    return (Γ + C).imag / 2          # :134


def cn_Vxx(Γ, C=None):
    """src/utilities.jl:126-129: the upper Cholesky factor of the block (Julia returns the ``Cholesky`` object)."""
    return _chol_upper(cn_fVxx(Γ, C))


def cn_Vyy(Γ, C=None):
    return _chol_upper(cn_fVyy(Γ, C))


def cn_Vxy(Γ, C=None):
    return _chol_upper(cn_fVxy(Γ, C))


def cn_Vyx(Γ, C=None):
    return _chol_upper(cn_fVyx(Γ, C))


def cn_Vs(Γ, C=None):
    return cn_Vxx(Γ, C), cn_Vyy(Γ, C), cn_Vxy(Γ, C), cn_Vyx(Γ, C)   # :136


def cn_fV(Γ, C=None):
    return np.block([[cn_fVxx(Γ, C), cn_fVxy(Γ, C)], [cn_fVyx(Γ, C), cn_fVyy(Γ, C)]])   # :137


def cn_V(Γ, C=None):
    """src/utilities.jl:138: ``cholesky(Hermitian(cn_fV(Γ,C)))``, its upper factor (host; :func:`rand` factors on the device)."""
    return _chol_upper(cn_fV(Γ, C))


def Σ(cn):
    """src/utilities.jl:139, as written (the reference's own ``# TODO: check this``): ``Matrix(cn.Γ)``."""
    return np.array(cn.Γ, copy=True)


_COV_DEVICE_ROWS = 4096   # sample matrices with at least this many rows are centred and reduced on the device (lpvs_cov_f64)


def _cov_columns(A, device):
    """``mean(A, dims=1)`` and ``cov(A)`` (corrected) of a tall matrix.  A few rows are small dense host algebra; the reference's own
    10⁶ × 6 case goes through the fixed-order reduction kernels of csrc/cnormal.hip."""
    A = np.asfortranarray(A, dtype=np.float64)
    rows, cols = A.shape
    if rows < _COV_DEVICE_ROWS:
        return A.mean(axis=0), np.atleast_2d(np.cov(A, rowvar=False, ddof=1))
    mean, Cm = np.zeros(cols), np.zeros((cols, cols), order="F")
    check(lib().lpvs_cov_f64(out_ptr(A), rows, cols, int(device), out_ptr(mean), out_ptr(Cm)))
    return mean, Cm


class ComplexNormal:
    """src/utilities.jl:83-111.  Fields ``m`` (complex n), ``Γ`` (n × n, Hermitian; kept as a matrix and factored lazily) and ``C``
    (n × n, complex symmetric).  The reference's four constructors:

    * ``ComplexNormal(X, Y)``: real sample matrices of equal shape (rows are samples), ``V = cov([X Y])``;
    * ``ComplexNormal(Xc)``: a complex sample matrix;
    * ``ComplexNormal(m, V)``: a real mean of length 2n (``[re; im]``) and the real 2n × 2n covariance;
    * ``ComplexNormal(mc, V)``: a complex mean of length n and the same V.

    Built from V, the instance remembers V: :func:`rand` factors it directly (``cn_fV(cn_V2ΓC(V)) == V`` to rounding)."""

    def __init__(self, a, b=None, device=0):
        self._V = None
        a = _host_c(a)
        if b is None:
            if not np.iscomplexobj(a):
                raise TypeError("ComplexNormal(X): X must be complex (use ComplexNormal(X, Y) for real sample matrices)")
            a, b = a.real, a.imag                                             # :97-99
        else:
            b = _host_c(b)
        if a.shape == b.shape and not (a.ndim == 1 and b.ndim == 2):          # (X, Y)  :89-95
            X, Y = np.atleast_2d(a.T).T, np.atleast_2d(b.T).T
            mean, V = _cov_columns(np.concatenate([X, Y], axis=1), device)
            n = X.shape[1]
            self.m = mean[:n] + 1j * mean[n:]
            self._V = _sym_upper(V)
        else:                                                                 # (m, V)  :101-111
            if a.ndim != 1 or b.ndim != 2 or b.shape[0] != b.shape[1]:
                raise ValueError("ComplexNormal(m, V): m must be a vector and V a square matrix")
            if np.iscomplexobj(a):
                self.m = np.array(a, dtype=np.complex128)
            else:
                if len(a) % 2:
                    raise ValueError("ComplexNormal(m, V): a real mean needs an even length ([re; im])")   # Int(length(m)/2): InexactError
                n = len(a) // 2
                self.m = a[:n] + 1j * a[n:]
            if b.shape[0] != 2 * len(self.m):
                raise ValueError(f"ComplexNormal(m, V): V is {b.shape[0]} x {b.shape[1]}, the mean has {len(self.m)} complex components")
            self._V = _sym_upper(np.asarray(b, dtype=np.float64))
        self.Γ, self.C = cn_V2ΓC(self._V)

    @classmethod
    def from_parts(cls, m, Γ, C):
        """The inner constructor ``ComplexNormal(m, Γ, C)`` (:83-87)."""
        self = cls.__new__(cls)
        self._V = None
        self.m, self.Γ, self.C = np.asarray(m, dtype=np.complex128), _herm_upper(np.asarray(Γ, dtype=np.complex128)), _sym_upper(np.asarray(C, dtype=np.complex128))
        return self

    def covariance(self):
        """The real 2n × 2n covariance in ``[re; im]`` order: the V the instance was built from, else ``cn_fV(Γ, C)``."""
        return self._V if self._V is not None else cn_fV(self.Γ, self.C)


def _host_c(a):
    """A host array that keeps a complex eltype."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if np.iscomplexobj(a) else a.astype(np.float64, copy=False)


def pdf(cn, z):
    """src/utilities.jl:151-163, the formula as written (``conj(Γ) = Γ`` is the reference's own remark)."""
    Γ, Cc, m = cn.Γ, cn.C, cn.m
    z = np.asarray(z, dtype=np.complex128)
    k = len(m)
    U = _chol_upper(Γ)                                                        # the lazily taken factor: PosDefException here
    Γinv = np.linalg.inv(Γ)
    R = np.conj(Cc).conj().T @ Γinv
    P = Γ - R @ Cc
    zmm, czmm = z - m, np.conj(z) - np.conj(m)
    ld = np.concatenate([np.conj(czmm), np.conj(zmm)])
    rd = np.concatenate([zmm, czmm])
    S = np.block([[Γ, Cc], [np.conj(Cc), Γ]])
    detΓ = float(np.prod(np.diag(U).real) ** 2)                               # det(::Cholesky)
    return 1 / (np.pi ** k * np.sqrt(detΓ * np.linalg.det(P) + 0j)) * np.exp(-0.5 * (ld @ np.linalg.solve(S, rd)))


def affine_transform(cn, A, b):
    """src/utilities.jl:165."""
    A = np.asarray(A)
    return ComplexNormal.from_parts(A @ cn.m + np.asarray(b), A @ cn.Γ @ np.conj(A.T), A @ cn.C @ A.T)


def _normals_arg(normals, s, n2):
    """(keepalive, pointer) of a caller-supplied s × 2n matrix of standard normals, column-major on its own side (host or device)."""
    if normals is None:
        return None, None
    if tuple(normals.shape) != (s, n2):
        raise ValueError(f"normals must be {s} x {n2}, got {tuple(normals.shape)}")
    if _lib.is_device_array(normals):
        k, p, _ = as_f64(normals.t().contiguous())                           # row-major 2n × s == column-major s × 2n
        return k, p
    k, p, _ = as_f64(normals)
    return k, p


class _CnHandle:
    """The device side of a ComplexNormal: V factored once, the factor resident (lpvs_cn_create_f64)."""

    def __init__(self, m, V, device):
        m = np.asarray(m, dtype=np.complex128)
        self.n = len(m)
        mre, mim = np.ascontiguousarray(m.real), np.ascontiguousarray(m.imag)
        kv, pv, cnt = as_f64(V)
        if cnt != 4 * self.n * self.n:
            raise ValueError(f"the covariance must be {2 * self.n} x {2 * self.n}")
        h = C.c_int64(0)
        check(lib().lpvs_cn_create_f64(out_ptr(mre), out_ptr(mim), pv, self.n, int(device), C.byref(h)))
        self.h = h.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.h:
            lib().lpvs_cn_destroy(C.c_int64(self.h))
            self.h = 0
        return False


def rand(cn, s, seed=0, normals=None, device=0):
    """``rand(cn, s)`` (src/utilities.jl:168-174): s draws, an s × n complex matrix.  ``z = m' .+ R·U`` with U the upper Cholesky
    factor of the real covariance, on the device.  R is ``normals`` (s × 2n, numpy or a float64 device tensor) or, when ``None``, the
    library's own counter-based stream of ``seed`` (:func:`randn`); Julia's ``randn`` stream is not reproduced."""
    s = int(s)
    if s < 1:
        raise ValueError("the number of draws must be positive")
    kr, pr = _normals_arg(normals, s, 2 * len(cn.m))
    with _CnHandle(cn.m, cn.covariance(), device) as h:
        zr, zi = np.zeros((s, h.n), order="F"), np.zeros((s, h.n), order="F")
        check(lib().lpvs_cn_rand_f64(h.h, s, int(seed), pr, out_ptr(zr), out_ptr(zi)))
    return zr + 1j * zi


def randn(rows, cols, seed=0, row0=0, device=0):
    """Rows ``row0 … row0+rows−1`` of the library's standard-normal matrix of ``seed`` (numpy, rows × cols): element (i, j) depends on
    (seed, i, j) only -- Philox4x32-10, Box–Muller (include/lpvspectral.h g3)."""
    R = np.zeros((int(rows), int(cols)), order="F")
    check(lib().lpvs_randn_f64(int(seed), int(row0), int(rows), int(cols), int(device), out_ptr(R)))
    return R


def cholesky_upper(V, device=0):
    """U (upper, U'U = V) of a symmetric positive definite matrix on the device; only the upper triangle of V is read.
    :class:`NumericError` (PosDefException) when a pivot is not positive."""
    kv, pv, cnt = as_f64(V)
    n2 = int(round(np.sqrt(cnt)))
    if n2 * n2 != cnt or n2 < 1:
        raise ValueError("V must be a square matrix")
    U = np.zeros((n2, n2), order="F")
    check(lib().lpvs_cholesky_upper_f64(pv, n2, int(device), out_ptr(U)))
    return U


def cn_last_timing():
    """HIP-event times (ms) of this thread's last ComplexNormal device calls."""
    o = np.zeros(8)
    check(lib().lpvs_cn_last_timing(out_ptr(o), 8))
    return dict(factor_ms=o[0], sample_ms=o[1], bands_ms=o[2], total_ms=o[3], n2=int(o[4]), draws=int(o[5]), cells=int(o[6]))


@dataclass
class SchedFunc:
    """What the ``SpectralExt`` plot recipe computes (src/plotting.jl:54-106): ``F``/``P`` the amplitude and phase of the estimated
    dependence on the grid ``v`` (Nf × G), ``FBl``/``FBu``/``FBm`` the 10 % / 90 % Monte-Carlo bands and the mean of the draws,
    ``PB*`` the same of the phase.  ``line`` is what the recipe plots (``FBm`` when ``mcmean`` and bands exist, else ``F``)."""
    w: Any
    v: Any
    F: Any
    P: Any
    FBl: Any
    FBu: Any
    FBm: Any
    PBl: Any
    PBu: Any
    PBm: Any
    mcmean: bool = False

    @property
    def line(self):
        return self.FBm if (self.mcmean and self.FBm is not None) else self.F   # src/plotting.jl:129


def _linrange(a, b, n):
    """``LinRange(a, b, n)``: element i is ``(1 - t) a + t b`` with ``t = i / (n - 1)`` (Julia's lerpi)."""
    t = np.arange(n) / (n - 1)
    return (1 - t) * a + t * b


def schedfunc(se, normalization="none", normdim="freq", bounds=True, nMC=5000, phase=False, mcmean=False, seed=0, normals=None, device=0):
    """The numbers of ``plot(se::SpectralExt; normalization, normdim, bounds, nMC, phase, mcmean)`` (src/plotting.jl:54-106) ->
    :class:`SchedFunc`.  The grid is ``LinRange(min V, max V, 101 if Nf == 100 else 100)``; ``F[j,i] = |dot(x[j,:], ϕ(v_i))|`` and
    ``P = angle(...)`` (Julia's ``dot`` conjugates its first argument).  With ``bounds`` and ``se.Σ``: nMC draws of
    ``ComplexNormal(se.x, se.Σ)`` on the device, the 0-based order statistics ``nMC//10 − 1`` and ``nMC − nMC//10 − 1`` and the mean
    per (frequency, grid point), selected in LDS -- the ``FB[Nf, G, nMC]`` array of the reference never exists.  Bands are ``None``
    without ``bounds`` or without Σ; ``PB*`` stay zero unless ``phase`` (as the reference leaves them).

    As in the reference (:99-106), ``normalization`` (``"sum"`` / ``"max"`` along ``normdim`` ``"freq"`` / ``"v"``) divides ``F`` only:
    the bands are NOT normalised there, and are not here.

    ``normals`` (nMC × 2n) replaces the library's own stream of ``seed``."""
    w = _host_vec(se.w)
    Nf, Nv = len(w), int(se.Nv)
    x = reshape_params(np.asarray(se.x, dtype=np.complex128), Nf)
    nb = x.shape[1]
    Vh = _host(se.V)
    G = 101 if Nf == 100 else 100
    vg = _linrange(float(Vh.min()), float(Vh.max()), G)
    # the grid has the minimum, maximum and largest magnitude of V, so the activation kernel places the centres of K = basis_activation_func(V, ...)
    Φg = basis_activation_func(vg, Nv, se.normalize, se.coulomb)
    if Φg.shape[1] != nb:
        raise ValueError(f"se.x has {nb} coefficients per frequency, the basis has {Φg.shape[1]} functions")
    d = np.conj(x) @ Φg.T
    F, P = np.abs(d), np.angle(d)
    nMC = int(nMC)
    FBl = FBu = FBm = PBl = PBu = PBm = None
    if bounds and se.Σ is not None:
        if nMC < 10:
            raise ValueError(f"nMC must be at least 10 (the lower band is draw nMC ÷ 10 of the sort), got {nMC}")
        kr, pr = _normals_arg(normals, nMC, 2 * Nf * nb)
        out = [np.zeros((Nf, G), order="F") for _ in range(6)]
        with _CnHandle(np.asarray(se.x, dtype=np.complex128).ravel(), se.Σ, device) as h:
            ptrs = [out_ptr(o) for o in out[:3]] + [out_ptr(o) if phase else None for o in out[3:]]
            check(lib().lpvs_cn_bands_f64(h.h, Nf, nb, out_ptr(Φg), G, nMC, int(seed), pr, int(bool(phase)), *ptrs))
        FBl, FBu, FBm, PBl, PBu, PBm = out
    if normalization != "none":
        nd = 0 if normdim == "freq" else 1
        if normalization == "sum":
            F = F / (F.sum(axis=nd, keepdims=True) / F.shape[nd])
        elif normalization == "max":
            F = F / F.max(axis=nd, keepdims=True)
        else:
            raise ValueError(f"normalization must be 'none', 'sum' or 'max', got {normalization!r}")
    return SchedFunc(w, vg, F, P, FBl, FBu, FBm, PBl, PBu, PBm, bool(mcmean))


def detrend_(x, order=0, t=None):
    """``detrend!(x, order=0, t=1:length(x))`` (src/utilities.jl:1-8), in place on a numpy array or a torch tensor (on its own
    device).  Order 1 is the reference AS WRITTEN (:4-5): ``k = x \\ t`` is the scalar ``(x·t)/(x·x)`` of the centred x and
    ``x -= k·t`` -- this is not the least-squares slope of x over t."""
    if hasattr(x, "detach") and hasattr(x, "dtype") and not isinstance(x, np.ndarray):
        import torch
        x -= x.mean()
        if order == 1:
            tt = torch.arange(1, x.numel() + 1, dtype=x.dtype, device=x.device) if t is None else torch.as_tensor(t, dtype=x.dtype, device=x.device)
            x -= (torch.dot(x, tt) / torch.dot(x, x)) * tt
        return x
    if not isinstance(x, np.ndarray) or x.ndim != 1:
        raise TypeError("detrend_ works in place on a 1-D numpy array or torch tensor")
    xf = x.astype(np.float64) - np.mean(x)
    if order == 1:
        tt = np.arange(1, len(x) + 1, dtype=np.float64) if t is None else np.asarray(t, dtype=np.float64)
        xf = xf - (np.dot(xf, tt) / np.dot(xf, xf)) * tt
    if x.dtype.kind in "iu":
        if not np.array_equal(np.rint(xf), xf):
            raise ValueError("InexactError: the detrended values are not integers (detrend! on an integer vector)")
    x[:] = xf
    return x


def detrend(x, order=0, t=None):
    """``detrend(x, order=0, t=1:length(x))`` (src/utilities.jl:14-17): a detrended copy; see :func:`detrend_` for order 1."""
    if hasattr(x, "clone"):
        return detrend_(x.clone(), order, t)
    y = np.array(x, copy=True)
    if y.dtype.kind not in "iuf":
        y = y.astype(np.float64)
    return detrend_(y, order, t)
