# LPVSpectralAMD.jl -- reference-side binding of liblpvspectral.so (include/lpvspectral.h).
#
# Drop-in replacement of the hot path of LPVSpectral.jl (src/lsfft.jl, src/lasso.jl, src/windows.jl): same function
# names, positional arguments and keywords; the arithmetic runs in hand-written HIP kernels on MI355X through @ccall.
# NOT EXECUTABLE in the build image (no julia there).  It is written against the C-ABI, mirrors the Python host code in
# lpvspectral.jl_amd/api.py that the parity tests exercise, and every @ccall below is checked -- symbol, arity and
# argument types -- against the ctypes signature table by tests/test_julia_binding.py.
#
# Conventions used throughout (INTEGRATION.md section 5):
#   * every array handed to the library is first converted to a dense Vector / Matrix of the ABI's eltype, bound to a
#     local name, and that LOCAL is what GC.@preserve protects (never a temporary);
#   * the library never calls back into Julia: progress lines, cb(x,z) and Ctrl-C are handled here between chunks.
module LPVSpectralAMD

using Printf, LinearAlgebra, Statistics
import ProximalOperators                       # the reference's own prox objects are the dispatch types (src/lasso.jl:1)
const PO = ProximalOperators

export ls_spectral, tls_spectral, ls_sparse_spectral, ls_sparse_spectral_lpv, ls_spectral_lpv, ls_windowpsd, ls_windowcsd,
       ls_cohere, ls_windowpsd_lpv, get_fourier_regressor, check_freq, default_freqs, Windows2, Windows3, mapwindows,
       SpectralExt, psd, reshape_params, ADMM, rect, hanning, autocov, autocor, isequidistant,
       melspectrogram, mfcc, mel, spectrogram, Spectrogram, MelSpectrogram, MFCC, freq, rand_cn, schedfunc,
       Periodogram, welch_pgram, periodogram, compress, heatmap, predict, residual, fva, lombscargle, lombscargle_last_timing, lombscargle_terms_last_timing,
       lombscargle_spectrogram, lombscargle_welch, lombscargle_windows_last_timing, time_windows, wwz, wwz_radius, wwz_last_timing, bls, bls_frequencies, bls_last_timing, pdm, aov, conditional_entropy, pdm_last_timing, cent_last_timing, dirty_spectrum, clean_loop, clean_restore, clean, clean_sigma, clean_last_timing, lombscargle_bootstrap,
       lombscargle_bootstrap_last_timing

const LIB = get(ENV, "LPVSPECTRAL_LIB", joinpath(@__DIR__, "..", "lpvspectral.jl_amd", "liblpvspectral.so"))

# ---- status codes -> the exceptions the reference throws --------------------------------------
struct NumericError <: Exception; msg::String; end        # (G + shift I) not positive definite / singular normal equations
last_error() = unsafe_string(@ccall LIB.lpvs_last_error()::Cstring)
function check(rc::Int32)
    rc == 0 && return nothing
    msg = last_error()
    rc == -1 && throw(ArgumentError(msg))                 # src/lsfft.jl:22
    rc == -2 && throw(AssertionError(msg))                # src/lasso.jl:143, src/windows.jl:31
    rc == -3 && throw(DomainError(msg))                   # DSP.arraysplit: noverlap >= n
    rc == -4 && throw(OutOfMemoryError())
    rc == -7 && throw(NumericError(msg))
    error("lpvspectral ($rc): $msg")
end

const EST_SPARSE = Int32(1)                               # LPVS_EST_SPARSE
const EST_DENSE = Int32(2)                                # LPVS_EST_DENSE
const EST_SPARSE_INIT = Int32(3)                          # LPVS_EST_SPARSE_INIT: init = true, x0 = fourier_solve(A, y, zerofreq, λ)

# ---- ProximalOperators objects -> the four device prox kinds -----------------------------------
# Field names are those of ProximalOperators.jl 0.10-0.16 (`lambda`, `r`, `fs`, `idxs`) [PO-recalled, SURVEY.md section 8(c)];
# anything else -- or a sliced sum that is not equal-length contiguous NormL2 groups -- has no device kernel: `nothing`
# makes the callers fall back to the reference's own Julia ADMM.
proxparams(g::PO.NormL1, n) = g.lambda isa Real ? (Int32(1), Float64(g.lambda), Int64(0)) : nothing
proxparams(g::PO.NormL0, n) = (Int32(2), Float64(g.lambda), Int64(0))
proxparams(g::PO.IndBallL0, n) = (Int32(3), Float64(g.r), Int64(0))
function proxparams(g::PO.SlicedSeparableSum, n)          # src/lasso.jl:53-55: Nf groups ((f-1)L+1:fL,), all NormL2(λ)
    length(g.fs) == 1 || return nothing
    fs, idxs = g.fs[1], g.idxs[1]
    (eltype(fs) <: PO.NormL2 && !isempty(fs)) || return nothing
    λ = fs[1].lambda
    all(f -> f.lambda == λ, fs) || return nothing
    L = length(idxs[1][1])
    for (k, ix) in enumerate(idxs)
        (length(ix) == 1 && ix[1] == ((k - 1) * L + 1):(k * L)) || return nothing
    end
    length(idxs) * L <= n || return nothing
    (Int32(4), Float64(λ), Int64(L))
end
proxparams(g, n) = nothing

struct SpectralExt                                         # src/LPVSpectral.jl:59-70
    Y; X; V; w; Nv; λ; coulomb::Bool; normalize::Bool; x; Σ
end
reshape_params(x, Nf) = reshape(x, Nf, :)                  # src/utilities.jl:77
psd(se::SpectralExt) = abs2.(sum(reshape_params(copy(se.x), length(se.w)), dims=2))   # src/lsfft.jl:214-217

default_freqs(n::Int, fs=1) = (0:(n >> 1)) .* (fs / n)     # src/lsfft.jl:3-9 (rfftfreq)
default_freqs(t::AbstractVector, fs=1/mean(diff(t))) = default_freqs(length(t), fs)
default_freqs(t::AbstractVector, n::Int) = default_freqs(t[1:n])

rect(n) = ones(n)                                          # DSP.rect
hanning(n) = n > 1 ? 0.5 .* (1 .+ cos.(2π .* range(-0.5, 0.5, length=n))) : ones(1)   # DSP.hanning

dense(::Type{T}, a) where T = a isa Vector{T} ? a : Vector{T}(vec(collect(a)))

function check_freq(f)                                     # src/lsfft.jl:20-24
    fv = dense(Float64, f); z = Ref{Int64}(0)
    GC.@preserve fv check(@ccall LIB.lpvs_check_freq_f64(fv::Ptr{Float64}, length(fv)::Int64, z::Ref{Int64})::Int32)
    z[] == 0 ? nothing : Int(z[])
end

function get_fourier_regressor(t::AbstractArray{T}, f::AbstractArray{T}) where T   # src/lsfft.jl:26-49
    tv, fv = dense(Float64, t), dense(Float64, f)
    zf = check_freq(fv)
    A = zeros(Float64, length(tv), zf === nothing ? 2length(fv) : 2length(fv) - 1)
    z = Ref{Int64}(0)
    GC.@preserve tv fv A check(@ccall LIB.lpvs_fourier_regressor_f64(tv::Ptr{Float64}, length(tv)::Int64,
        fv::Ptr{Float64}, length(fv)::Int64, A::Ptr{Float64}, z::Ref{Int64})::Int32)
    T.(A), zf
end

# Float32 method (the reference is eltype-generic): same call through the _f32 entry point, Float32 in and out
function get_fourier_regressor(t::AbstractArray{Float32}, f::AbstractArray{Float32})
    tv, fv = dense(Float32, t), dense(Float32, f)
    z = Ref{Int64}(0)
    GC.@preserve fv check(@ccall LIB.lpvs_check_freq_f32(fv::Ptr{Float32}, length(fv)::Int64, z::Ref{Int64})::Int32)
    zf = z[] == 0 ? nothing : Int(z[])
    A = zeros(Float32, length(tv), zf === nothing ? 2length(fv) : 2length(fv) - 1)
    GC.@preserve tv fv A check(@ccall LIB.lpvs_fourier_regressor_f32(tv::Ptr{Float32}, length(tv)::Int64,
        fv::Ptr{Float32}, length(fv)::Int64, A::Ptr{Float32}, z::Ref{Int64})::Int32)
    A, zf
end

# ---- options (include/lpvspectral.h LPVS_OPT_*) ---------------------------------------------------
# Extensions (the reference has none of them): how a handle stores the inverse its ADMM mat-vec streams and how it iterates.
#   storage   = :mixed (>= 36 significant bits per element, all read every iteration; 1e-10 in the iterates) | :split (40 bits) | :f64 (doubles) |
#               :mixed32 (the default of single-signal handles with n >= 2048: :mixed's tiles, of which the iteration reads 32 bits; the 4-bit
#               planes ride, up to 32 iterations stale, in the x-update's offset vector -- x, z, u as with :mixed: include/lpvspectral.h)
#   iteration = :one (default where applicable: one launch per ADMM iteration) | :two
#   gram_form = :ap | :krs | :kr,  nt_loads = :on | :off,  slot_sums = :nufft | :direct        (`nothing` = the library's choice)
# Estimators take them as keywords (`ls_sparse_spectral_lpv(...; storage=:f64)`); results do not depend on them beyond rounding.
#   window_chunk_mb = MB of packed inverses per chunk of the batched-window engine | :uncut;  windows_in_flight = 1 .. 4 parts of a chunk;
#   reserve_cus = CUs the factorisation leaves to its pivot chain | :none                     (integers; defaults only, not handle options)
const OPT_ID = (storage=Int32(1), iteration=Int32(2), gram_form=Int32(3), nt_loads=Int32(4), slot_sums=Int32(5),
                window_chunk_mb=Int32(6), windows_in_flight=Int32(7), reserve_cus=Int32(8), xupdate_correction=Int32(9))
const OPT_VALUES = (storage=(mixed=1, split=2, f64=3, mixed32=4), iteration=(one=1, two=2), gram_form=(ap=1, krs=2, kr=3),
                    nt_loads=(off=1, on=2), slot_sums=(nufft=1, direct=2), window_chunk_mb=(uncut=-1,), windows_in_flight=NamedTuple(),
                    reserve_cus=(none=-1,), xupdate_correction=(on=1, off=2))
optvalue(name::Symbol, v) = v === nothing ? Int32(0) : v isa Integer ? Int32(v) : Int32(getfield(getfield(OPT_VALUES, name), Symbol(v)))
function set_default_option(name::Symbol, v=nothing)       # thread-local: handles created / window batches run afterwards
    oid, vid = getfield(OPT_ID, name), optvalue(name, v)
    check(@ccall LIB.lpvs_set_default_option(oid::Int32, vid::Int32)::Int32)
end
function get_default_option(name::Symbol)
    oid = getfield(OPT_ID, name); r = Ref{Int32}(0)
    check(@ccall LIB.lpvs_get_default_option(oid::Int32, r::Ref{Int32})::Int32)
    r[] == 0 && return nothing
    vals = getfield(OPT_VALUES, name)
    for k in keys(vals); getfield(vals, k) == r[] && return k; end
    Int(r[])                                              # integer-valued options: the number itself
end
const OPTION_KEYS = keys(OPT_ID)
# run f() with the given option keywords as thread defaults, restore the previous defaults afterwards; returns the
# remaining keywords (the reference's own: iters, tol, μ, ...)
function with_options(f, kwargs)
    mine = [(k, v) for (k, v) in pairs(kwargs) if k in OPTION_KEYS && v !== nothing]
    prev = [(k, get_default_option(k)) for (k, _) in mine]
    for (k, v) in mine; set_default_option(k, v); end
    try
        return f((; (k => v for (k, v) in pairs(kwargs) if !(k in OPTION_KEYS))...))
    finally
        for (k, v) in prev; set_default_option(k, v); end
    end
end

# ---- handle wrapper ----------------------------------------------------------------------------
mutable struct Problem
    h::Ptr{Cvoid}; n::Int; m::Int; ns::Int                 # m = complex parameters per signal, ns = right-hand sides
    function Problem(h, m, ns=1)
        n = Ref{Int64}(0); check(@ccall LIB.lpvs_problem_size(h::Ptr{Cvoid}, n::Ref{Int64})::Int32)
        p = new(h, Int(n[]), m, ns)
        finalizer(q -> (@ccall LIB.lpvs_problem_destroy(q.h::Ptr{Cvoid})::Int32), p)
    end
end

function set_option!(p::Problem, name::Symbol, v=nothing)  # one handle; takes effect at the next admm init / run
    oid, vid = getfield(OPT_ID, name), optvalue(name, v)
    check(@ccall LIB.lpvs_problem_set_option(p.h::Ptr{Cvoid}, oid::Int32, vid::Int32)::Int32)
end
function get_option(p::Problem, name::Symbol)              # the value in effect (explicit, thread default or environment)
    oid = getfield(OPT_ID, name); r = Ref{Int32}(0)
    check(@ccall LIB.lpvs_problem_get_option(p.h::Ptr{Cvoid}, oid::Int32, r::Ref{Int32})::Int32)
    r[] == 0 ? nothing : keys(getfield(OPT_VALUES, name))[r[]]
end

function fourier_problem(y, t, f, W; device=0)
    yv, tv, fv = dense(Float64, y), dense(Float64, t), dense(Float64, f)
    @assert length(yv) == length(tv) "y and t has to be the same length"
    Wv = W === nothing ? Float64[] : dense(Float64, W)     # a named local: stays alive under GC.@preserve
    @assert W === nothing || length(Wv) == length(yv) "W has to be the same length as y"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve yv tv fv Wv check(@ccall LIB.lpvs_problem_create_fourier_f64(yv::Ptr{Float64}, tv::Ptr{Float64},
        length(yv)::Int64, fv::Ptr{Float64}, length(fv)::Int64, Wp::Ptr{Float64}, Int32(device)::Int32, h::Ref{Ptr{Cvoid}})::Int32)
    Problem(h[], length(fv))
end

function lpv_problem(y, X, V, w, Nv, normalize, coulomb; device=0)
    yv, Xv, Vv, wv = dense(Float64, y), dense(Float64, X), dense(Float64, V), dense(Float64, w)
    @assert length(yv) == length(Xv) == length(Vv) "y, X and V has to be the same length"
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve yv Xv Vv wv check(@ccall LIB.lpvs_problem_create_lpv_f64(yv::Ptr{Float64}, Xv::Ptr{Float64},
        Vv::Ptr{Float64}, length(yv)::Int64, wv::Ptr{Float64}, length(wv)::Int64, Int64(Nv)::Int64, Int32(normalize)::Int32,
        Int32(coulomb)::Int32, Int32(device)::Int32, h::Ref{Ptr{Cvoid}})::Int32)
    Problem(h[], length(wv) * (coulomb ? 2Nv : Nv))
end

# Y is N x ns (one column per signal sharing X, V, w): one Gram, ns right-hand sides
function lpv_multi_problem(Y::AbstractMatrix, X, V, w, Nv, normalize, coulomb; device=0)
    Ym = Matrix{Float64}(Y); Xv, Vv, wv = dense(Float64, X), dense(Float64, V), dense(Float64, w)
    @assert size(Ym, 1) == length(Xv) == length(Vv) "Y, X and V has to have the same number of samples"
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Ym Xv Vv wv check(@ccall LIB.lpvs_problem_create_lpv_multi_f64(Ym::Ptr{Float64}, size(Ym, 2)::Int64,
        Xv::Ptr{Float64}, Vv::Ptr{Float64}, size(Ym, 1)::Int64, wv::Ptr{Float64}, length(wv)::Int64, Int64(Nv)::Int64,
        Int32(normalize)::Int32, Int32(coulomb)::Int32, Int32(device)::Int32, h::Ref{Ptr{Cvoid}})::Int32)
    Problem(h[], length(wv) * (coulomb ? 2Nv : Nv), size(Ym, 2))
end

function dense_problem(A::AbstractMatrix, y; device=0)    # ADMM(x, LeastSquares(A, y; iterative=true), proxg)
    Am, yv = Matrix{Float64}(A), dense(Float64, y)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Am yv check(@ccall LIB.lpvs_problem_create_dense_f64(Am::Ptr{Float64}, yv::Ptr{Float64}, size(Am, 1)::Int64,
        size(Am, 2)::Int64, C_NULL::Ptr{Float64}, Int32(device)::Int32, h::Ref{Ptr{Cvoid}})::Int32)
    Problem(h[], 0)
end
function gram_problem(Q::AbstractMatrix, q; device=0)     # ADMM(x, Quadratic(Q, q; iterative=true), proxg)
    Qm, qv = Matrix{Float64}(Q), dense(Float64, q)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Qm qv check(@ccall LIB.lpvs_problem_create_gram_f64(Qm::Ptr{Float64}, qv::Ptr{Float64}, size(Qm, 1)::Int64,
        Int32(device)::Int32, h::Ref{Ptr{Cvoid}})::Int32)
    Problem(h[], 0)
end

# ---- regularisation path (extension): ns penalties on one shared inverse -----------------------
# a handle with ns signal slots from a single-signal problem of any constructor: a copy of its Gram, ns copies of its right-hand side
function path_problem(src::Problem, ns::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(@ccall LIB.lpvs_problem_create_path(src.h::Ptr{Cvoid}, Int64(ns)::Int64, h::Ref{Ptr{Cvoid}})::Int32)
    Problem(h[], src.m, Int(ns))
end
# pars[q] is the λ (or the r of IndBallL0) of signal slot q; kind and glen as in proxparams
function set_prox_per_signal!(p::Problem, kind::Integer, pars, glen::Integer=0)
    pv = dense(Float64, pars)
    GC.@preserve pv check(@ccall LIB.lpvs_problem_set_prox_per_signal(p.h::Ptr{Cvoid}, Int32(kind)::Int32, pv::Ptr{Float64},
        Int64(length(pv))::Int64, Int64(glen)::Int64)::Int32)
end
function prox_params(p::Problem)                           # what every slot's prox will read (the scalar repeated if one prox is set)
    out = zeros(p.ns)
    GC.@preserve out check(@ccall LIB.lpvs_problem_get_prox_params(p.h::Ptr{Cvoid}, out::Ptr{Float64}, Int64(p.ns)::Int64)::Int32)
    out
end

function params(p::Problem, which=0)
    re, im_ = zeros(p.m * p.ns), zeros(p.m * p.ns)
    GC.@preserve re im_ check(@ccall LIB.lpvs_problem_get_params_f64(p.h::Ptr{Cvoid}, Int32(which)::Int32, re::Ptr{Float64}, im_::Ptr{Float64})::Int32)
    complex.(re, im_)
end
function pack(p::Problem, coef::Vector{Float64})
    re, im_ = zeros(p.m), zeros(p.m)
    GC.@preserve coef re im_ check(@ccall LIB.lpvs_problem_pack_params_f64(p.h::Ptr{Cvoid}, coef::Ptr{Float64}, re::Ptr{Float64}, im_::Ptr{Float64})::Int32)
    complex.(re, im_)
end
function solve_ridge(p::Problem, ridge)
    x = zeros(p.n)
    GC.@preserve x check(@ccall LIB.lpvs_problem_solve_ridge_f64(p.h::Ptr{Cvoid}, Float64(ridge)::Float64, x::Ptr{Float64})::Int32)
    x
end
function gram(p::Problem)
    G = zeros(p.n, p.n); b = zeros(p.n)
    GC.@preserve G b check(@ccall LIB.lpvs_problem_get_gram_f64(p.h::Ptr{Cvoid}, G::Ptr{Float64}, b::Ptr{Float64})::Int32)
    G, b
end
function rhs(p::Problem)
    B = zeros(p.n, p.ns)
    GC.@preserve B check(@ccall LIB.lpvs_problem_get_rhs_f64(p.h::Ptr{Cvoid}, B::Ptr{Float64})::Int32)
    B
end
function inverse(p::Problem, shift)
    M = zeros(p.n, p.n)
    GC.@preserve M check(@ccall LIB.lpvs_problem_get_inverse_f64(p.h::Ptr{Cvoid}, Float64(shift)::Float64, M::Ptr{Float64})::Int32)
    M
end
function inverse_refined(p::Problem, shift)                 # one round of iterative refinement on the device, symmetrised: an inverse that is the result
    M = zeros(p.n, p.n)
    GC.@preserve M check(@ccall LIB.lpvs_problem_get_inverse_refined_f64(p.h::Ptr{Cvoid}, Float64(shift)::Float64, M::Ptr{Float64})::Int32)
    (M .+ M') ./ 2
end
function iterates(p::Problem)
    x, z, u = zeros(p.n, p.ns), zeros(p.n, p.ns), zeros(p.n, p.ns)
    GC.@preserve x z u check(@ccall LIB.lpvs_admm_get_f64(p.h::Ptr{Cvoid}, x::Ptr{Float64}, z::Ptr{Float64}, u::Ptr{Float64})::Int32)
    p.ns == 1 ? (vec(x), vec(z), vec(u)) : (x, z, u)
end
# resume (SURVEY.md section 5): install iterates saved by `iterates` into a freshly initialised handle
function set_state!(p::Problem, x, z, u, iters_done::Integer; offset=nothing)
    xv, zv, uv = dense(Float64, x), dense(Float64, z), dense(Float64, u)
    GC.@preserve xv zv uv check(@ccall LIB.lpvs_admm_set_state_f64(p.h::Ptr{Cvoid}, xv::Ptr{Float64}, zv::Ptr{Float64}, uv::Ptr{Float64},
        Int64(iters_done)::Int64)::Int32)
    if offset !== nothing          # the offset vector saved with the iterates (`offset_vector`): the run continues bit for bit
        ov = dense(Float64, offset)
        GC.@preserve ov check(@ccall LIB.lpvs_admm_set_offset_f64(p.h::Ptr{Cvoid}, ov::Ptr{Float64}, Int64(length(ov))::Int64)::Int32)
    end
end
# the x-update's offset vector currently in effect (handles of n >= 2048; `nothing` otherwise): part of a checkpoint next to `iterates`.
# Opaque: n x ns values, or 2n for a handle that iterates on 32-bit reads of its fixed-point tiles (lpvs_admm_offset_len).
function offset_vector(p::Problem)
    k = Ref{Int64}(0)
    check(@ccall LIB.lpvs_admm_offset_len(p.h::Ptr{Cvoid}, k::Ref{Int64})::Int32)
    k[] == 0 && return nothing
    xb = zeros(k[])
    GC.@preserve xb check(@ccall LIB.lpvs_admm_get_offset_f64(p.h::Ptr{Cvoid}, xb::Ptr{Float64}, Int64(length(xb))::Int64)::Int32)
    (p.ns == 1 || k[] != p.n * p.ns) ? xb : reshape(xb, p.n, p.ns)
end

# ---- ADMM driver: src/lasso.jl:136-171 with the iterations on the GPU ---------------------------
# One blocking @ccall per chunk of `printerval` iterations, so @printf/@info, cb(x,z) and Ctrl-C
# (InterruptException, src/lasso.jl:59-63) are all handled by Julia on the calling thread.
function admm!(p::Problem, x0, prox::Tuple, sign; iters=10000, tol=1e-5, printerval=100, cb=nothing, μ=0.05)
    @assert 0 ≤ μ ≤ 1 "μ should be ≤ 1"                                              # :143
    kind, par, glen = prox
    check(@ccall LIB.lpvs_problem_set_prox(p.h::Ptr{Cvoid}, kind::Int32, par::Float64, glen::Int64)::Int32)
    x0v = x0 === nothing ? Float64[] : dense(Float64, x0)
    x0p = x0 === nothing ? Ptr{Float64}(C_NULL) : pointer(x0v)
    GC.@preserve x0v check(@ccall LIB.lpvs_admm_init_f64(p.h::Ptr{Cvoid}, x0p::Ptr{Float64}, Float64(μ)::Float64,
        Float64(tol)::Float64, Int32(sign)::Int32)::Int32)
    done = 0; conv = false
    it, nxz, cv = Ref{Int64}(0), Ref{Float64}(0), Ref{Int32}(0)
    printerval = printerval > 0 ? printerval : iters
    while done < iters && !conv
        chunk = min(printerval - done % printerval, iters - done)
        check(@ccall LIB.lpvs_admm_run(p.h::Ptr{Cvoid}, Int64(chunk)::Int64, it::Ref{Int64}, nxz::Ref{Float64}, cv::Ref{Int32})::Int32)
        done, conv = Int(it[]), cv[] != 0
        if done % printerval == 0
            @printf("%d ||x-z||₂ %.10f\n", done, nxz[])                              # :159
            cb !== nothing && (xz = iterates(p); cb(xz[1], xz[2]))                   # :160-162
        end
        if conv
            @printf("%d ||x-z||₂ %.10f\n", done, nxz[])                              # :165
            @info("||x-z||₂ ≤ tol")                                                   # :166
        end
    end
    xz = iterates(p)
    xz[1], xz[2]
end

"""`x, z = ADMM(x, proxf, proxg; iters, tol, printerval, cb, μ)` (src/lasso.jl:136-171): `proxf` a
`ProximalOperators.LeastSquares(A, b; iterative=true)` or `Quadratic(Q, q; iterative=true)`, `proxg` one of the four device
prox kinds; anything else is not accelerated (call the reference's ADMM)."""
function ADMM(x::AbstractArray{T}, proxf, proxg; iters=10000, tol=1e-5, printerval=100, cb=nothing, μ=T(0.05)) where T
    kwargs = (iters=iters, tol=tol, printerval=printerval, cb=cb, μ=μ)
    pp = proxparams(proxg, length(x))
    pp === nothing && throw(ArgumentError("proxg of type $(typeof(proxg)) has no device kernel"))
    # field names of the iterative variants [PO-recalled]: LeastSquaresIterative(A, b, lambda...), QuadraticIterative(Q, q)
    if hasproperty(proxf, :A) && hasproperty(proxf, :b)
        x_, z_ = admm!(dense_problem(proxf.A, proxf.b), x, pp, +1; kwargs...)
    elseif hasproperty(proxf, :Q) && hasproperty(proxf, :q)
        x_, z_ = admm!(gram_problem(proxf.Q, proxf.q), x, pp, -1; kwargs...)        # (Q + I/μ) x = -q + v/μ
    else
        throw(ArgumentError("proxf of type $(typeof(proxf)) has no device path"))
    end
    copyto!(x, x_)                                                                    # the reference mutates x in place (:151)
    x, z_
end

# ---- estimators: same signatures as the reference ------------------------------------------------
function ls_spectral(y, t, f=default_freqs(t); λ=1e-10, verbose=false, device=0)     # src/lsfft.jl:62-67
    yv, tv, fv = dense(Float64, y), dense(Float64, t), dense(Float64, f)
    @assert length(yv) == length(tv) "y and t has to be the same length"
    re, im_ = zeros(length(fv)), zeros(length(fv))
    # [A; λI] \ [y; 0] from the device Gram in its better-conditioned form (primal for tall, dual for fat systems such as the
    # default grid of an even-length record, whose Gram is singular): lpvs_ls_spectral_f64, NOT a ridge solve with λ²
    try
        GC.@preserve yv tv fv re im_ check(@ccall LIB.lpvs_ls_spectral_f64(yv::Ptr{Float64}, tv::Ptr{Float64}, length(yv)::Int64,
            fv::Ptr{Float64}, length(fv)::Int64, Float64(λ)::Float64, Int32(device)::Int32, re::Ptr{Float64}, im_::Ptr{Float64})::Int32)
    catch e
        e isa NumericError || rethrow(e)                  # normal equations singular to working precision: the reference's QR route on the host
        A, zf = get_fourier_regressor(tv, fv)
        x = [A; λ * I] \ [yv; zeros(size(A, 2))]
        nf = length(fv)
        re .= x[1:nf]
        im_ .= zf === nothing ? x[nf+1:end] : [0.0; x[nf+1:end]]   # fourier2complex, src/utilities.jl:62-73
    end
    if verbose                                                                       # :65
        G, _ = gram(fourier_problem(yv, tv, fv, nothing; device=device))
        @info("Condition number: $(round(cond(G), digits=2))\n")
    end
    complex.(re, im_), f
end
function ls_spectral(y, t, f, W::AbstractVector; verbose=false, λ=1e-10, device=0)   # src/lsfft.jl:74-80
    p = fourier_problem(y, t, f, W; device=device)
    x = pack(p, solve_ridge(p, λ))                       # (A'WA + λI) \ A'Wy
    verbose && @info("Condition number: $(round(cond(gram(p)[1]), digits=2))\n")      # :78
    x, f
end

function tls_spectral(y, t, f=default_freqs(t)[1:end-1])                               # src/lsfft.jl:85-99
    p = fourier_problem(y, t, f, nothing)
    G, b = gram(p)
    H = [G b; b' dot(y, y)]                             # [A y]'[A y]: its smallest eigenvector is the last right singular vector
    v = eigen(Symmetric(H)).vectors[:, 1]
    pack(p, -v[1:p.n] ./ v[p.n + 1]), f
end

_x0(q, zf) = zf === nothing ? [real.(q); imag.(q)] : [real.(q); imag.(q[2:end])]     # src/lasso.jl:93-97

function ls_sparse_spectral(y::AbstractArray{T}, t, f=default_freqs(t); init=false, λ=T(1),
                            proxg=PO.NormL1(λ), device=0, kwargs...) where T          # src/lasso.jl:85-102
    with_options(kwargs) do kw                           # storage= / iteration= ... (extensions) apply to the handle created here
        p = fourier_problem(y, t, f, nothing; device=device)
        pp = proxparams(proxg, p.n)
        pp === nothing && throw(ArgumentError("proxg of type $(typeof(proxg)) has no device kernel; use LPVSpectral.ls_sparse_spectral"))
        x0 = init ? _x0(pack(p, solve_ridge(p, λ^2)), check_freq(f)) : nothing       # fourier_solve(A,y,zerofreq,λ), :92
        admm!(p, x0, pp, +1; kw...)
        params(p), f
    end
end
function ls_sparse_spectral(y::AbstractArray{T}, t, f, W; init=false, λ=T(1), proxg=PO.NormL1(T(λ)), device=0,
                            kwargs...) where T                                       # src/lasso.jl:105-126
    with_options(kwargs) do kw
        p = fourier_problem(y, t, f, W; device=device)
        pp = proxparams(proxg, p.n)
        pp === nothing && throw(ArgumentError("proxg of type $(typeof(proxg)) has no device kernel; use LPVSpectral.ls_sparse_spectral"))
        x0 = init ? _x0(ls_spectral(y, t, f; λ=λ, device=device)[1], check_freq(f)) : nothing   # :112 -- the UNWEIGHTED solve
        admm!(p, x0, pp, -1; kw...)                       # Quadratic(Q, q=+A'Wy) as written (:119-121)
        params(p), f
    end
end

function ls_sparse_spectral_lpv(y::AbstractVector{S}, X::AbstractVector{S}, V::AbstractVector{S}, w, Nv::Integer;
                                λ=1, coulomb=false, normalize=true, device=0, kwargs...) where S   # src/lasso.jl:27-70
    coulomb && throw(ArgumentError("coulomb=true is ill-defined in the sparse LPV path (half of x is never written by prox!); use ls_spectral_lpv"))
    w = w[:]
    with_options(kwargs) do kw
        p = lpv_problem(y, X, V, w, Nv, normalize, false; device=device)
        local prm
        try
            admm!(p, nothing, (Int32(4), Float64(λ), Int64(2Nv)), +1; kw...)        # SlicedSeparableSum(NormL2(λ)...), :53-55
            prm = params(p, 0)
        catch e
            e isa InterruptException || rethrow(e)
            @info "Aborting"                              # :61
            prm = params(p, 1)                            # z = copy(x)
        end
        SpectralExt(y, X, V, w, Nv, λ, coulomb, normalize, prm, nothing)
    end
end

# Multichannel batch over several devices (extension; BASELINE.json config 5): the columns of Y (N x ns) share X, V, w; contiguous
# channel ranges go to `ngpus` devices driven by this one process (ngpus = 0: every visible device).  proxg = nothing gives the
# reference's frequency-grouped lasso (src/lasso.jl:53-55) per channel.  Returns a Vector of SpectralExt.
function ls_sparse_spectral_lpv(Y::AbstractMatrix{S}, X::AbstractVector{S}, V::AbstractVector{S}, w, Nv::Integer;
                                λ=1, normalize=true, proxg=nothing, iters=10000, tol=1e-5, μ=0.05, ngpus=0) where S
    @assert 0 ≤ μ ≤ 1 "μ should be ≤ 1"
    w = w[:]
    Ym = Matrix{Float64}(Y); Xv, Vv, wv = dense(Float64, X), dense(Float64, V), dense(Float64, w)
    N, ns = size(Ym); Nf = length(wv); m = Nf * Nv
    @assert N == length(Xv) == length(Vv) "Y, X and V has to have the same number of samples"
    pp = proxg === nothing ? (Int32(4), Float64(λ), Int64(2Nv)) : proxparams(proxg, 2Nf * Nv)
    pp === nothing && throw(ArgumentError("proxg of type $(typeof(proxg)) has no device kernel"))
    re, im_ = zeros(m, ns), zeros(m, ns); its = zeros(Int64, ns)
    GC.@preserve Ym Xv Vv wv re im_ its check(@ccall LIB.lpvs_lpv_batch_multi_f64(Ym::Ptr{Float64}, Int64(ns)::Int64, Xv::Ptr{Float64}, Vv::Ptr{Float64},
        Int64(N)::Int64, wv::Ptr{Float64}, Int64(Nf)::Int64, Int64(Nv)::Int64, Int32(normalize)::Int32, pp[1]::Int32, pp[2]::Float64, pp[3]::Int64,
        Float64(μ)::Float64, Float64(tol)::Float64, Int64(iters)::Int64, C_NULL::Ptr{Int32}, Int32(ngpus)::Int32, re::Ptr{Float64}, im_::Ptr{Float64},
        its::Ptr{Int64})::Int32)
    [SpectralExt(Ym[:, q], X, V, w, Nv, λ, false, normalize, complex.(re[:, q], im_[:, q]), nothing) for q in 1:ns]
end

# Independent signals (extension; BASELINE.json config 3 as a batch): column q of Y, X and V (all N x nsig) is one signal with its own
# samples, i.e. the loop [ls_sparse_spectral_lpv(Y[:,q], X[:,q], V[:,q], w, Nv; ...) for q] inside the library -- contiguous signal
# ranges over `ngpus` devices, `in_flight` solves at a time per device, each on its own handle and stream (the matrix-core-bound Gram /
# factorisation of one solve under the HBM-bound iterations of another).  Returns a Vector of SpectralExt.
function ls_sparse_spectral_lpv(Y::AbstractMatrix{S}, X::AbstractMatrix{S}, V::AbstractMatrix{S}, w, Nv::Integer;
                                λ=1, normalize=true, proxg=nothing, iters=10000, tol=1e-5, μ=0.05, ngpus=0, in_flight=2) where S
    @assert 0 ≤ μ ≤ 1 "μ should be ≤ 1"
    w = w[:]
    Ym, Xm, Vm = Matrix{Float64}(Y), Matrix{Float64}(X), Matrix{Float64}(V); wv = dense(Float64, w)
    N, nsig = size(Ym); Nf = length(wv); m = Nf * Nv
    @assert size(Xm) == size(Vm) == (N, nsig) "Y, X and V has to have the same number of samples"
    pp = proxg === nothing ? (Int32(4), Float64(λ), Int64(2Nv)) : proxparams(proxg, 2Nf * Nv)
    pp === nothing && throw(ArgumentError("proxg of type $(typeof(proxg)) has no device kernel"))
    re, im_ = zeros(m, nsig), zeros(m, nsig); its = zeros(Int64, nsig)
    GC.@preserve Ym Xm Vm wv re im_ its check(@ccall LIB.lpvs_lpv_signals_multi_f64(Ym::Ptr{Float64}, Xm::Ptr{Float64}, Vm::Ptr{Float64},
        Int64(N)::Int64, Int64(nsig)::Int64, wv::Ptr{Float64}, Int64(Nf)::Int64, Int64(Nv)::Int64, Int32(normalize)::Int32, pp[1]::Int32, pp[2]::Float64,
        pp[3]::Int64, Float64(μ)::Float64, Float64(tol)::Float64, Int64(iters)::Int64, C_NULL::Ptr{Int32}, Int32(ngpus)::Int32, Int32(in_flight)::Int32,
        re::Ptr{Float64}, im_::Ptr{Float64}, its::Ptr{Int64})::Int32)
    [SpectralExt(Ym[:, q], Xm[:, q], Vm[:, q], w, Nv, λ, false, normalize, complex.(re[:, q], im_[:, q]), nothing) for q in 1:nsig]
end

function ls_spectral_lpv(Y::AbstractVector, X::AbstractVector, V::AbstractVector, w, Nv::Integer;
                         λ=1e-8, coulomb=false, normalize=true, device=0, covariance=true)   # src/lsfft.jl:239-259
    w = w[:]
    Yv = dense(Float64, Y); N = length(Yv)
    if !covariance                                          # (extension: ls_windowpsd_lpv reads the parameters only -- no Σ, no second inverse)
        p1 = lpv_problem(Yv, X, V, w, Nv, normalize, coulomb; device=device)
        x1 = try solve_ridge(p1, λ^2) catch e; e isa NumericError || rethrow(e); nothing end
        x1 === nothing || return SpectralExt(Y, X, V, w, Nv, λ, coulomb, normalize, pack(p1, x1), nothing)
    end
    p = lpv_multi_problem([Yv ones(N)], X, V, w, Nv, normalize, coulomb; device=device)   # second right-hand side: the constant signal
    Nf, nb = length(w), coulomb ? 2Nv : Nv
    local x
    try
        x = solve_ridge(p, λ^2)                           # real_complex_bs(A, Y, λ) in normal-equation form, permuted column order
    catch e
        e isa NumericError || rethrow(e)                  # (G + λ²I) singular to working precision: the reference's QR route on the host
        Φ = zeros(N, 2Nf * nb)
        Xv, Vv, wv = dense(Float64, X), dense(Float64, V), dense(Float64, w)
        GC.@preserve Xv Vv wv Φ check(@ccall LIB.lpvs_lpv_regressor_f64(Xv::Ptr{Float64}, Vv::Ptr{Float64}, Int64(N)::Int64, wv::Ptr{Float64},
            Int64(Nf)::Int64, Int64(Nv)::Int64, Int32(normalize)::Int32, Int32(coulomb)::Int32, Int32(1)::Int32, Φ::Ptr{Float64})::Int32)
        x = [Φ; λ * I] \ [Yv; zeros(2Nf * nb)]
    end
    prm = pack(p, x)
    G, _ = gram(p); B = rhs(p)
    e2 = dot(x, G * x) - 2dot(B[:, 1], x) + dot(Yv, Yv)   # ‖AA·x − Y‖² from the Gram
    esum = dot(B[:, 2], x) - sum(Yv)                      # Σe through the constant right-hand side
    var_e = (e2 - esum^2 / N) / (N - 1)                   # var(e), :253
    Minv = try inverse_refined(p, λ) catch e; e isa NumericError || rethrow(e); inv(G + λ * I) end   # inv(AA'AA + λI), λ as written
    # reference order u = c·Nf·nb + j·Nf + f  <-  device order q = f·2nb + c·nb + j   (0-based c, j, f)
    perm = Vector{Int}(undef, 2Nf * nb)
    for f in 0:Nf-1, c in 0:1, j in 0:nb-1
        perm[c * Nf * nb + j * Nf + f + 1] = f * 2nb + c * nb + j + 1
    end
    Σ = var_e .* Minv[perm, perm]
    fva = 1 - var_e / var(Yv)                             # :255
    fva < 0.9 && @warn("Fraction of variance explained = $(fva)")                    # :256
    SpectralExt(Y, X, V, w, Nv, λ, coulomb, normalize, prm, Σ)
end

# ---- model evaluation (extension: the reference has no predict): the regressor times the coefficients without the regressor ------
# path = :auto | :direct (any frequency grid) | :nufft (a type-2 non-uniform FFT; grids that are an arithmetic progression up to rounding)
const EVAL_PATHS = Dict(:auto => Int32(0), :direct => Int32(1), :nufft => Int32(2))
_columns(x) = (P = reshape(ComplexF64.(x), size(x, 1), :); (Matrix{Float64}(real.(P)), Matrix{Float64}(imag.(P)), size(P, 2)))
_shaped(x, out) = x isa AbstractVector ? vec(out) : out
# -> (ŷ or y − ŷ as M × nc, [Σ Σ²] of every output column as nc × 2); the basis is the FITTED one: centres from the ranges of se.V
function _eval_lpv(se::SpectralExt, X, V, y, path::Symbol, device)
    wv, Xv, Vv, Vt = dense(Float64, se.w), dense(Float64, X), dense(Float64, V), dense(Float64, se.V)
    Nf, M = length(wv), length(Xv)
    @assert length(Vv) == M "X and V has to be the same length"
    pre, pim, nc = _columns(se.x)
    ranges = Float64[minimum(Vt), maximum(Vt), maximum(abs, Vt)]
    out, sums = zeros(M, nc), zeros(2, nc)
    if y === nothing
        GC.@preserve pre pim wv ranges Xv Vv out sums check(@ccall LIB.lpvs_lpv_eval_f64(pre::Ptr{Float64}, pim::Ptr{Float64}, Int64(nc)::Int64, wv::Ptr{Float64}, Int64(Nf)::Int64, Int64(se.Nv)::Int64, Int32(se.normalize)::Int32, Int32(se.coulomb)::Int32, ranges::Ptr{Float64}, Xv::Ptr{Float64}, Vv::Ptr{Float64}, C_NULL::Ptr{Float64}, Int64(M)::Int64, EVAL_PATHS[path]::Int32, Int32(device)::Int32, out::Ptr{Float64}, sums::Ptr{Float64})::Int32)
    else
        yv = dense(Float64, y)
        @assert length(yv) == M "y has to be as long as the sampling points"
        GC.@preserve pre pim wv ranges Xv Vv yv out sums check(@ccall LIB.lpvs_lpv_eval_f64(pre::Ptr{Float64}, pim::Ptr{Float64}, Int64(nc)::Int64, wv::Ptr{Float64}, Int64(Nf)::Int64, Int64(se.Nv)::Int64, Int32(se.normalize)::Int32, Int32(se.coulomb)::Int32, ranges::Ptr{Float64}, Xv::Ptr{Float64}, Vv::Ptr{Float64}, yv::Ptr{Float64}, Int64(M)::Int64, EVAL_PATHS[path]::Int32, Int32(device)::Int32, out::Ptr{Float64}, sums::Ptr{Float64})::Int32)
    end
    out, permutedims(sums)
end
function _eval_fourier(x, f, t, y, path::Symbol, device)
    fv, tv = dense(Float64, f), dense(Float64, t)
    Nf, M = length(fv), length(tv)
    pre, pim, nc = _columns(x)
    @assert size(pre, 1) == Nf "one complex coefficient per frequency (what ls_spectral returns)"
    out, sums = zeros(M, nc), zeros(2, nc)
    if y === nothing
        GC.@preserve pre pim fv tv out sums check(@ccall LIB.lpvs_fourier_eval_f64(pre::Ptr{Float64}, pim::Ptr{Float64}, Int64(nc)::Int64, fv::Ptr{Float64}, Int64(Nf)::Int64, tv::Ptr{Float64}, C_NULL::Ptr{Float64}, Int64(M)::Int64, EVAL_PATHS[path]::Int32, Int32(device)::Int32, out::Ptr{Float64}, sums::Ptr{Float64})::Int32)
    else
        yv = dense(Float64, y)
        @assert length(yv) == M "y has to be as long as the sampling points"
        GC.@preserve pre pim fv tv yv out sums check(@ccall LIB.lpvs_fourier_eval_f64(pre::Ptr{Float64}, pim::Ptr{Float64}, Int64(nc)::Int64, fv::Ptr{Float64}, Int64(Nf)::Int64, tv::Ptr{Float64}, yv::Ptr{Float64}, Int64(M)::Int64, EVAL_PATHS[path]::Int32, Int32(device)::Int32, out::Ptr{Float64}, sums::Ptr{Float64})::Int32)
    end
    out, permutedims(sums)
end
_fva(sums, M, y) = 1 .- ((sums[:, 2] .- sums[:, 1] .^ 2 ./ M) ./ (M - 1)) ./ var(dense(Float64, y))   # src/lsfft.jl:255, var(e) from the device's sums
_scalar(x, v) = x isa AbstractVector ? v[1] : v

"""    predict(se::SpectralExt, X=se.X, V=se.V; path=:auto)   and   predict(x, f, t; path=:auto)
The fitted model at the samples: `lpv_regressor(X, V, …, permuted=false) * [real(x); imag(x)]` resp. `get_fourier_regressor(t, f)[1] * x`
without the regressor; a matrix of coefficient columns (a regularisation path) gives one output column each."""
predict(se::SpectralExt, X=se.X, V=se.V; path::Symbol=:auto, device=0) = _shaped(se.x, _eval_lpv(se, X, V, nothing, path, device)[1])
predict(x::AbstractVecOrMat, f::AbstractVector, t::AbstractVector; path::Symbol=:auto, device=0) = _shaped(x, _eval_fourier(x, f, t, nothing, path, device)[1])
"    residual(se) = se.Y − predict(se)   and   residual(x, f, t, y) = y − predict(x, f, t), formed on the device"
residual(se::SpectralExt; path::Symbol=:auto, device=0) = _shaped(se.x, _eval_lpv(se, se.X, se.V, se.Y, path, device)[1])
residual(x::AbstractVecOrMat, f::AbstractVector, t::AbstractVector, y::AbstractVector; path::Symbol=:auto, device=0) = _shaped(x, _eval_fourier(x, f, t, y, path, device)[1])
"    fva(se)   and   fva(x, f, t, y): fraction of variance explained, 1 − var(e)/var(y) (src/lsfft.jl:255), one value per coefficient column"
fva(se::SpectralExt; path::Symbol=:auto, device=0) = _scalar(se.x, _fva(_eval_lpv(se, se.X, se.V, se.Y, path, device)[2], length(se.Y), se.Y))
fva(x::AbstractVecOrMat, f::AbstractVector, t::AbstractVector, y::AbstractVector; path::Symbol=:auto, device=0) = _scalar(x, _fva(_eval_fourier(x, f, t, y, path, device)[2], length(y), y))
function eval_last_timing()
    tm = zeros(10)
    GC.@preserve tm check(@ccall LIB.lpvs_eval_last_timing(tm::Ptr{Float64}, Int32(10)::Int32)::Int32)
    (path=Int(tm[1]), nf=Int(tm[2]), twin=tm[3] != 0, stage_ms=tm[4], grid_ms=tm[5], eval_ms=tm[6], sums_ms=tm[7], copy_ms=tm[8], total_ms=tm[9], slabs=Int(tm[10]))
end

# ---- windows: src/windows.jl (offsets from the C-ABI, views into the arrays) ---------------------
abstract type AbstractWindows end
function _offsets(L::Int, n::Int, noverlap::Int)
    k = Ref{Int64}(0)
    check(@ccall LIB.lpvs_window_count(Int64(L)::Int64, Int64(n)::Int64, Int64(noverlap)::Int64, k::Ref{Int64})::Int32)
    off = zeros(Int64, max(k[], 1))
    GC.@preserve off check(@ccall LIB.lpvs_window_offsets(Int64(L)::Int64, Int64(n)::Int64, Int64(noverlap)::Int64, off::Ptr{Int64},
        Int64(length(off))::Int64, k::Ref{Int64})::Int32)
    off[1:k[]]
end
struct Windows2 <: AbstractWindows; y; t; n::Int; noverlap::Int; W; offsets::Vector{Int64}; end
function Windows2(y::AbstractVector, t::AbstractVector, n::Int=length(y) >> 3, noverlap::Int=n >> 1, window_func=rect)   # :27-36
    noverlap < 0 && (noverlap = n >> 1)
    @assert length(y) == length(t) "y and t has to be the same length"
    Windows2(y, t, n, noverlap, eltype(y).(window_func(n)), _offsets(length(y), n, noverlap))
end
struct Windows3 <: AbstractWindows; y; t; v; n::Int; noverlap::Int; W; offsets::Vector{Int64}; end
function Windows3(y::AbstractVector, t::AbstractVector, v::AbstractVector, n::Int=length(y) >> 3, noverlap::Int=n >> 1, window_func=rect)   # :94-103
    @assert length(y) == length(t) == length(v) "y, t and v has to be the same length"
    noverlap < 0 && (noverlap = n >> 1)
    Windows3(y, t, v, n, noverlap, window_func(n), _offsets(length(y), n, noverlap))
end
Base.length(w::AbstractWindows) = length(w.offsets)
_rng(w, s) = (w.offsets[s] + 1):(w.offsets[s] + w.n)
Base.iterate(w::Windows2, s=1) = s > length(w) ? nothing : ((view(w.y, _rng(w, s)), view(w.t, _rng(w, s))), s + 1)
Base.iterate(w::Windows3, s=1) = s > length(w) ? nothing : ((view(w.y, _rng(w, s)), view(w.t, _rng(w, s)), view(w.v, _rng(w, s))), s + 1)

function merge(yf::AbstractVector{<:AbstractVector}, w::AbstractWindows)              # src/windows.jl:57-70
    flat = zeros(Float64, w.n, length(w))
    for (i, v) in enumerate(yf); flat[:, i] .= v; end    # column i = window i: the ABI's window-major layout
    ym = zeros(length(w.y))
    GC.@preserve flat ym check(@ccall LIB.lpvs_merge_f64(flat::Ptr{Float64}, Int64(length(w))::Int64, Int64(w.n)::Int64, Int64(w.noverlap)::Int64,
        Int64(length(w.y))::Int64, ym::Ptr{Float64})::Int32)
    ym
end
mapwindows(f::Function, W::AbstractWindows) = merge([f(w) for w in W], W)             # :50-53
mapwindows(f::Function, args...) = mapwindows(f, Windows2(args...))

# ---- the batched-window engine: all windows of the drivers below in ONE call ---------------------
# Which estimator / kwargs combinations the engine covers (everything else runs the reference's sequential loop):
#   estimator === ls_spectral         (the 4-argument weighted method, src/lsfft.jl:74-80)    kwargs ⊆ (λ,)
#   estimator === ls_sparse_spectral  (the 4-argument weighted method, src/lasso.jl:105-126)  no cb; init = true and all four device prox kinds included
function engine_args(estimator, nreg; kwargs...)
    kw = Dict{Symbol,Any}(kwargs)
    delete!(kw, :device)
    for k in OPTION_KEYS; delete!(kw, k); end                # (applied as thread defaults by the drivers)
    if estimator === ls_spectral
        (get(kw, :verbose, false) || !issubset(keys(kw), (:λ, :verbose))) && return nothing
        return (est=EST_DENSE, lam=Float64(get(kw, :λ, 1e-10)), prox=(Int32(1), 0.0, Int64(0)), μ=0.05, tol=0.0, iters=0, sign=Int32(1))
    elseif estimator === ls_sparse_spectral
        get(kw, :cb, nothing) !== nothing && return nothing                          # a per-iteration callback needs the host loop
        issubset(keys(kw), (:λ, :proxg, :μ, :tol, :iters, :printerval, :cb, :init)) || return nothing
        g = get(kw, :proxg, PO.NormL1(Float64(get(kw, :λ, 1.0))))
        pp = proxparams(g, nreg)
        pp === nothing && return nothing
        μ = Float64(get(kw, :μ, 0.05))
        @assert 0 ≤ μ ≤ 1 "μ should be ≤ 1"
        init = Bool(get(kw, :init, false))                                           # src/lasso.jl:112: one batched ridge solve in the engine
        return (est=init ? EST_SPARSE_INIT : EST_SPARSE, lam=init ? Float64(get(kw, :λ, 1.0)) : 0.0, prox=pp, μ=μ,
                tol=Float64(get(kw, :tol, 1e-5)), iters=Int(get(kw, :iters, 10000)), sign=Int32(-1))
    end
    nothing
end

# x[Nf, k, ns] complex: column (·, i, s) = fourier2complex of window i of signal s; `ngpus` devices are driven by this one
# process (contiguous window ranges per device, one RCCL all-gather of the coefficients; ngpus = 0: every visible device)
function windows_estimate(Ys::Vector, t, freqs, n::Int, noverlap::Int, W, eng; ngpus::Int=1)
    L = length(Ys[1]); ns = length(Ys)
    Ym = Matrix{Float64}(undef, L, ns)
    for (s, y) in enumerate(Ys); Ym[:, s] .= y; end
    tv, fv, Wv = dense(Float64, t), dense(Float64, freqs), dense(Float64, W)
    k = length(_offsets(L, n, noverlap)); Nf = length(fv)
    re, im_ = zeros(Nf, k, ns), zeros(Nf, k, ns)          # column-major (Nf, k, ns) == the ABI's ns x k x Nf
    its = zeros(Int64, k, ns)
    GC.@preserve Ym tv fv Wv re im_ its check(@ccall LIB.lpvs_windows_estimate_multi_f64(Ym::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64},
        Int64(L)::Int64, Int64(n)::Int64, Int64(noverlap)::Int64, Wv::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, eng.est::Int32,
        eng.lam::Float64, eng.prox[1]::Int32, eng.prox[2]::Float64, eng.prox[3]::Int64, eng.μ::Float64, eng.tol::Float64,
        Int64(eng.iters)::Int64, eng.sign::Int32, C_NULL::Ptr{Int32}, Int32(ngpus)::Int32, re::Ptr{Float64}, im_::Ptr{Float64},
        its::Ptr{Int64})::Int32)
    complex.(re, im_), its
end

# The raw ADMM state of every window instead of the packed coefficients: (x, z) as `ADMM` returns them (src/lasso.jl:170) and the scaled dual
# variable u, each Nreg x k x ns (Nreg = 2Nf, or 2Nf - 1 with the zero frequency first; the reference's ordering [re; im], src/lasso.jl:93-97),
# and the iteration counts.  Sparse estimators, one device.  (What the parity tests hold the window batches' iteration to the CPU reference with.)
function windows_estimate_state(Ys::Vector, t, freqs, n::Int, noverlap::Int, W, eng; device::Int=0)
    L = length(Ys[1]); ns = length(Ys)
    Ym = Matrix{Float64}(undef, L, ns)
    for (s, y) in enumerate(Ys); Ym[:, s] .= y; end
    tv, fv, Wv = dense(Float64, t), dense(Float64, freqs), dense(Float64, W)
    k = length(_offsets(L, n, noverlap)); Nf = length(fv)
    nreg = check_freq(fv) === nothing ? 2Nf : 2Nf - 1
    x, z, u = zeros(nreg, k, ns), zeros(nreg, k, ns), zeros(nreg, k, ns)     # column-major (Nreg, k, ns) == the ABI's ns x k x Nreg
    its = zeros(Int64, k, ns)
    GC.@preserve Ym tv fv Wv x z u its check(@ccall LIB.lpvs_windows_estimate_state_f64(Ym::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64},
        Int64(L)::Int64, Int64(n)::Int64, Int64(noverlap)::Int64, Wv::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, eng.est::Int32,
        eng.lam::Float64, eng.prox[1]::Int32, eng.prox[2]::Float64, eng.prox[3]::Int64, eng.μ::Float64, eng.tol::Float64,
        Int64(eng.iters)::Int64, eng.sign::Int32, Int64(0)::Int64, Int64(k)::Int64, Int32(device)::Int32, x::Ptr{Float64}, z::Ptr{Float64},
        u::Ptr{Float64}, its::Ptr{Int64})::Int32)
    x, z, u, its
end

function ls_windowpsd(y, t, freqs=nothing; nw=8, noverlap=-1, window_func=rect, estimator=ls_spectral, ngpus=1, kwargs...)
    n = length(y) ÷ nw                                                               # src/lsfft.jl:112-126
    freqs === nothing && (freqs = default_freqs(t, n))
    windows = Windows2(y, t, n, noverlap, window_func)
    nw = length(windows)                                                             # :116 (recomputed)
    S = zeros(eltype(y), length(freqs))
    eng = nw > 0 ? engine_args(estimator, 2length(freqs); kwargs...) : nothing
    if eng !== nothing
        x, _ = with_options(kwargs) do _; windows_estimate([y], t, freqs, n, windows.noverlap, windows.W, eng; ngpus=ngpus); end
        for i in 1:nw
            S .+= abs2.(view(x, :, i, 1))                                            # :122, window order
        end
        return S ./ nw^2, freqs                                                      # :125
    end
    for (yi, ti) in windows
        x = estimator(yi, ti, freqs, windows.W; kwargs...)[1]                        # :121
        S .+= abs2.(x)
    end
    S ./ nw^2, freqs
end

function ls_windowcsd(y, u, t, freqs=nothing; nw=10, noverlap=-1, window_func=rect, estimator=ls_spectral, ngpus=1, kwargs...)
    n = length(y) ÷ nw                                                               # src/lsfft.jl:140-156
    freqs === nothing && (freqs = default_freqs(t, n))
    S = zeros(ComplexF64, length(freqs))
    windowsy = Windows2(y, t, n, noverlap, window_func)
    windowsu = Windows2(u, t, n, noverlap, window_func)
    nw = length(windowsy)
    eng = nw > 0 ? engine_args(estimator, 2length(freqs); kwargs...) : nothing
    if eng !== nothing                                    # one Gram and one factorisation per window serve both signals
        x, _ = with_options(kwargs) do _; windows_estimate([y, u], t, freqs, n, windowsy.noverlap, windowsy.W, eng; ngpus=ngpus); end
        for i in 1:nw
            S += view(x, :, i, 1) .* conj.(view(x, :, i, 2))                         # :152
        end
        return S ./ nw, freqs
    end
    for ((yi, ti), (ui, _)) in zip(windowsy, windowsu)
        xy = estimator(yi, ti, freqs, windowsy.W; kwargs...)[1]
        xu = estimator(ui, ti, freqs, windowsu.W; kwargs...)[1]
        S += xy .* conj.(xu)
    end
    S ./ nw, freqs
end

function ls_cohere(y, u, t, freqs=nothing; nw=10, noverlap=-1, estimator=ls_spectral, ngpus=1, kwargs...)
    n = length(y) ÷ nw                                                               # src/lsfft.jl:176-193
    freqs === nothing && (freqs = default_freqs(t, n))
    Syy, Suu = zeros(length(freqs)), zeros(length(freqs))
    Syu = zeros(ComplexF64, length(freqs))
    windows = Windows3(y, t, u, n, noverlap, hanning)                                # :182
    eng = length(windows) > 0 ? engine_args(estimator, 2length(freqs); kwargs...) : nothing
    if eng !== nothing
        x, _ = with_options(kwargs) do _; windows_estimate([y, u], t, freqs, n, windows.noverlap, windows.W, eng; ngpus=ngpus); end
        for i in 1:length(windows)
            xy, xu = view(x, :, i, 1), view(x, :, i, 2)
            Syu .+= xy .* conj.(xu); Syy .+= abs2.(xy); Suu .+= abs2.(xu)           # :187-189
        end
        return abs2.(Syu) ./ (Suu .* Syy), freqs
    end
    for (yi, ti, ui) in windows
        xy = estimator(yi, ti, freqs, windows.W; kwargs...)[1]
        xu = estimator(ui, ti, freqs, windows.W; kwargs...)[1]
        Syu .+= xy .* conj.(xu); Syy .+= abs2.(xy); Suu .+= abs2.(xu)
    end
    abs2.(Syu) ./ (Suu .* Syy), freqs
end

# The windows' regressors share nothing, so every window is a device solve of its own; `in_flight` of them (an extension; needs
# `julia -t N`) run concurrently, each on its own handle and stream -- statically scheduled, so a solve stays on the thread whose
# thread-local option defaults and error string it uses (defaults set with `set_default_option` on the calling thread do not reach the
# others: pass options as keywords).  The sum is taken in window order either way (src/lsfft.jl:274).
function ls_windowpsd_lpv(Y::AbstractVector, X::AbstractVector, V::AbstractVector, w, Nv::Integer, nw::Int=10, noverlap=0; in_flight::Int=4, kwargs...)
    S = zeros(length(w))                                                             # src/lsfft.jl:267-277
    # the library's own driver (the same device solves on the library's worker threads: no `julia -t` needed) whenever the call has only
    # what it takes; a singular window (NumericError) sends the call down the per-window path below, which has the host-QR route
    if all(k in (:λ, :coulomb, :normalize, :device) for k in keys(kwargs))
        @assert length(Y) == length(X) == length(V) "y, t and v has to be the same length"
        Yv, Xv, Vv, wv = dense(Float64, Y), dense(Float64, X), dense(Float64, V), dense(Float64, w[:])
        kw = (; kwargs...)
        kcnt = Ref{Int64}(0)
        check(@ccall LIB.lpvs_window_count(length(Yv)::Int64, Int64(length(Yv) ÷ nw)::Int64, Int64(noverlap)::Int64, kcnt::Ref{Int64})::Int32)
        fva = ones(max(kcnt[], 1))
        try
            GC.@preserve Yv Xv Vv wv S fva check(@ccall LIB.lpvs_windowpsd_lpv_f64(Yv::Ptr{Float64}, Xv::Ptr{Float64}, Vv::Ptr{Float64}, length(Yv)::Int64,
                wv::Ptr{Float64}, length(wv)::Int64, Int64(Nv)::Int64, Int64(length(Yv) ÷ nw)::Int64, Int64(noverlap)::Int64, Float64(get(kw, :λ, 1e-8))::Float64,
                Int32(get(kw, :normalize, true))::Int32, Int32(get(kw, :coulomb, false))::Int32, Int32(get(kw, :device, 0))::Int32,
                Int32(clamp(in_flight, 1, 8))::Int32, S::Ptr{Float64}, fva::Ptr{Float64})::Int32)
            for v in fva[1:kcnt[]]
                v < 0.9 && @warn("Fraction of variance explained = $(v)")            # src/lsfft.jl:255-256, per window
            end
            return S
        catch e
            e isa NumericError || rethrow()
            fill!(S, 0.0)
        end
    end
    windows = collect(Windows3(Y, X, V, length(Y) ÷ nw, noverlap, rect))
    solve((y, x, v)) = ls_spectral_lpv(collect(y), collect(x), collect(v), w, Nv; covariance=false, kwargs...)
    ses = Vector{Any}(undef, length(windows))
    if in_flight > 1 && Threads.nthreads() > 1 && length(windows) > 1
        nt = min(in_flight, Threads.nthreads())
        Threads.@threads :static for k in 1:nt
            for i in k:nt:length(windows)
                ses[i] = solve(windows[i])
            end
        end
    else
        for i in eachindex(windows)
            ses[i] = solve(windows[i])
        end
    end
    for se in ses
        S += vec(abs2.(sum(reshape_params(se.x, length(w)), dims=2)))
    end
    S
end

# ---- autocov / autocor at arbitrary sample times: src/autocov.jl (pairs, lag sums and the stable sort on the device) ----------
# Methods of this module's own functions (StatsBase's autocov(y) is not extended here: call LPVSpectralAMD.autocov when both are loaded).
isequidistant(v::AbstractRange) = step(v) > 0                                         # src/autocov.jl:112
function isequidistant(v::AbstractVector{<:Real})                                     # src/autocov.jl:113-121
    eq = Ref{Int32}(0)
    if eltype(v) == Float32
        v32 = Vector{Float32}(v)
        GC.@preserve v32 check(@ccall LIB.lpvs_isequidistant_f32(v32::Ptr{Float32}, Int64(length(v32))::Int64, eq::Ref{Int32})::Int32)
    else
        v64 = Vector{Float64}(v)
        GC.@preserve v64 check(@ccall LIB.lpvs_isequidistant_f64(v64::Ptr{Float64}, Int64(length(v64))::Int64, eq::Ref{Int32})::Int32)
    end
    eq[] != 0
end

# all segments in one call: the stable sort of (tau, segment, enumeration index) is what src/autocov.jl:1-12 returns
function _autofun(kind::Int32, t::AbstractVector, h::AbstractVector, maxlag::Real, normalize::Bool; device::Integer=0)
    length(t) == length(h) || throw(ArgumentError("t has $(length(t)) segments, y has $(length(h))"))
    all(length.(t) .== length.(h)) || throw(ArgumentError("t and y must be the same length"))   # src/autocov.jl:40
    tT = mapreduce(eltype, promote_type, t); yT = mapreduce(eltype, promote_type, h)
    f32 = tT == Float32 && yT == Float32
    off = Int64[0; cumsum(Int64.(length.(h)))]
    nseg = Int64(length(h)); n = Ref{Int64}(0)
    if f32
        t32 = Vector{Float32}(reduce(vcat, collect.(t))); y32 = Vector{Float32}(reduce(vcat, h))
        GC.@preserve t32 y32 off check(@ccall LIB.lpvs_autofun_f32(kind::Int32, t32::Ptr{Float32}, y32::Ptr{Float32}, off::Ptr{Int64}, nseg::Int64,
            Float64(maxlag)::Float64, Int32(normalize)::Int32, Int32(device)::Int32, C_NULL::Ptr{Float32}, C_NULL::Ptr{Float32}, Int64(0)::Int64,
            n::Ref{Int64})::Int32)
        tau32 = Vector{Float32}(undef, n[]); acf32 = Vector{Float32}(undef, n[])
        GC.@preserve t32 y32 off tau32 acf32 check(@ccall LIB.lpvs_autofun_f32(kind::Int32, t32::Ptr{Float32}, y32::Ptr{Float32}, off::Ptr{Int64},
            nseg::Int64, Float64(maxlag)::Float64, Int32(normalize)::Int32, Int32(device)::Int32, tau32::Ptr{Float32}, acf32::Ptr{Float32},
            Int64(length(tau32))::Int64, n::Ref{Int64})::Int32)
        return tau32, acf32
    end
    tT == Float32 && throw(ArgumentError("Float32 times with $(yT) values: pass both as Float32 or both as Float64"))
    t64 = Vector{Float64}(reduce(vcat, collect.(t))); y64 = Vector{Float64}(reduce(vcat, h))   # integer times: exact for |t| < 2^52
    GC.@preserve t64 y64 off check(@ccall LIB.lpvs_autofun_f64(kind::Int32, t64::Ptr{Float64}, y64::Ptr{Float64}, off::Ptr{Int64}, nseg::Int64,
        Float64(maxlag)::Float64, Int32(normalize)::Int32, Int32(device)::Int32, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64}, Int64(0)::Int64,
        n::Ref{Int64})::Int32)
    tau64 = Vector{Float64}(undef, n[]); acf64 = Vector{Float64}(undef, n[])
    GC.@preserve t64 y64 off tau64 acf64 check(@ccall LIB.lpvs_autofun_f64(kind::Int32, t64::Ptr{Float64}, y64::Ptr{Float64}, off::Ptr{Int64},
        nseg::Int64, Float64(maxlag)::Float64, Int32(normalize)::Int32, Int32(device)::Int32, tau64::Ptr{Float64}, acf64::Ptr{Float64},
        Int64(length(tau64))::Int64, n::Ref{Int64})::Int32)
    tT <: Integer ? round.(tT, tau64) : convert(Vector{tT}, tau64), convert(Vector{yT <: AbstractFloat ? yT : Float64}, acf64)
end

autocov(t::AbstractVector{<:Real}, y::AbstractVector{<:Real}, maxlag::Real; normalize=false, device=0) =       # src/autocov.jl:35
    _autofun(Int32(1), [t], [y], maxlag, Bool(normalize); device=device)
autocor(t::AbstractVector{<:Real}, y::AbstractVector{<:Real}, maxlag::Real; normalize=false, device=0) =       # src/autocov.jl:78
    _autofun(Int32(2), [t], [y], maxlag, Bool(normalize); device=device)
autocov(t::AbstractVector, h::AbstractVector{<:AbstractVector{<:Real}}, maxlag::Real; normalize=false, device=0) =   # src/autocov.jl:15
    _autofun(Int32(1), t, h, maxlag, Bool(normalize); device=device)
autocor(t::AbstractVector, h::AbstractVector{<:AbstractVector{<:Real}}, maxlag::Real; normalize=false, device=0) =   # src/autocov.jl:16
    _autofun(Int32(2), t, h, maxlag, Bool(normalize); device=device)

# ---- ComplexNormal draws and the Monte-Carlo bands of the SpectralExt recipe: src/utilities.jl:168-174, src/plotting.jl:54-106 --------
# The reference's ComplexNormal type stays the reference's (small host algebra); these two entry points take what it holds.
# rand_cn(m, V, s): s draws of the complex normal with mean m (complex n) and real 2n x 2n covariance V ([re; im] order), s x n.
# normals (s x 2n) replaces the library's own counter-based stream of `seed` (Julia's randn stream is not reproduced).
function _cn_create(m::AbstractVector{<:Complex}, V::AbstractMatrix{<:Real}, device::Integer)
    mre = Vector{Float64}(real.(m)); mim = Vector{Float64}(imag.(m)); V64 = Matrix{Float64}(V)
    size(V64) == (2length(mre), 2length(mre)) || throw(ArgumentError("V must be $(2length(mre)) x $(2length(mre))"))
    h = Ref{Int64}(0)
    GC.@preserve mre mim V64 check(@ccall LIB.lpvs_cn_create_f64(mre::Ptr{Float64}, mim::Ptr{Float64}, V64::Ptr{Float64},
        Int64(length(mre))::Int64, Int32(device)::Int32, h::Ref{Int64})::Int32)
    h[]
end
_cn_destroy(h::Int64) = (@ccall LIB.lpvs_cn_destroy(h::Int64)::Int32; nothing)

function rand_cn(m::AbstractVector{<:Complex}, V::AbstractMatrix{<:Real}, s::Integer; seed::Integer=0, normals=nothing, device::Integer=0)
    n = length(m)
    h = _cn_create(m, V, device)
    zre = Matrix{Float64}(undef, s, n); zim = Matrix{Float64}(undef, s, n)
    try
        if normals === nothing
            GC.@preserve zre zim check(@ccall LIB.lpvs_cn_rand_f64(h::Int64, Int64(s)::Int64, Int64(seed)::Int64, C_NULL::Ptr{Float64},
                zre::Ptr{Float64}, zim::Ptr{Float64})::Int32)
        else
            R64 = Matrix{Float64}(normals)
            size(R64) == (s, 2n) || throw(ArgumentError("normals must be $s x $(2n)"))
            GC.@preserve R64 zre zim check(@ccall LIB.lpvs_cn_rand_f64(h::Int64, Int64(s)::Int64, Int64(seed)::Int64, R64::Ptr{Float64},
                zre::Ptr{Float64}, zim::Ptr{Float64})::Int32)
        end
    finally
        _cn_destroy(h)
    end
    complex.(zre, zim)                                                                   # src/utilities.jl:173
end

# schedfunc(se; ...): the numbers of the plot recipe as a NamedTuple (w, v, F, P, FBl, FBu, FBm, PBl, PBu, PBm); the bands are `nothing`
# without bounds or without se.Σ, PB* stay zero unless phase, and normalization divides F only (src/plotting.jl:99-106, as written).
function schedfunc(se::SpectralExt; normalization=:none, normdim=:freq, bounds=true, nMC=5_000, phase=false, mcmean=false,
                   seed::Integer=0, normals=nothing, device::Integer=0)
    w = se.w[:]; Nf = length(w)
    x = reshape_params(ComplexF64.(se.x), Nf); nb = size(x, 2)
    G = Nf == 100 ? 101 : 100
    vg = Vector{Float64}(collect(LinRange(minimum(se.V), maximum(se.V), G)))             # src/plotting.jl:62
    Φg = Matrix{Float64}(undef, G, nb)
    GC.@preserve vg Φg check(@ccall LIB.lpvs_basis_activation_f64(vg::Ptr{Float64}, Int64(G)::Int64, Int64(se.Nv)::Int64,
        Int32(se.normalize)::Int32, Int32(se.coulomb)::Int32, Φg::Ptr{Float64})::Int32)
    d = conj.(x) * transpose(Φg)                                                         # dot(x[j,:], ϕ) conjugates x (:76)
    F = abs.(d); P = angle.(d)
    FBl = FBu = FBm = PBl = PBu = PBm = nothing
    if bounds && se.Σ !== nothing
        nMC >= 10 || throw(ArgumentError("nMC must be at least 10, got $nMC"))
        h = _cn_create(ComplexF64.(se.x[:]), se.Σ, device)
        FBl = zeros(Nf, G); FBu = zeros(Nf, G); FBm = zeros(Nf, G); PBl = zeros(Nf, G); PBu = zeros(Nf, G); PBm = zeros(Nf, G)
        try
            if normals === nothing
                GC.@preserve Φg FBl FBu FBm PBl PBu PBm check(@ccall LIB.lpvs_cn_bands_f64(h::Int64, Int64(Nf)::Int64, Int64(nb)::Int64,
                    Φg::Ptr{Float64}, Int64(G)::Int64, Int64(nMC)::Int64, Int64(seed)::Int64, C_NULL::Ptr{Float64}, Int32(phase)::Int32,
                    FBl::Ptr{Float64}, FBu::Ptr{Float64}, FBm::Ptr{Float64}, PBl::Ptr{Float64}, PBu::Ptr{Float64}, PBm::Ptr{Float64})::Int32)
            else
                R64 = Matrix{Float64}(normals)
                size(R64) == (nMC, 2Nf * nb) || throw(ArgumentError("normals must be $nMC x $(2Nf * nb)"))
                GC.@preserve Φg R64 FBl FBu FBm PBl PBu PBm check(@ccall LIB.lpvs_cn_bands_f64(h::Int64, Int64(Nf)::Int64, Int64(nb)::Int64,
                    Φg::Ptr{Float64}, Int64(G)::Int64, Int64(nMC)::Int64, Int64(seed)::Int64, R64::Ptr{Float64}, Int32(phase)::Int32,
                    FBl::Ptr{Float64}, FBu::Ptr{Float64}, FBm::Ptr{Float64}, PBl::Ptr{Float64}, PBu::Ptr{Float64}, PBm::Ptr{Float64})::Int32)
            end
        finally
            _cn_destroy(h)
        end
    end
    nd = normdim == :freq ? 1 : 2                                                        # :99
    if normalization == :sum
        F = F ./ (sum(F, dims=nd) / size(F, nd))                                         # :102
    elseif normalization == :max
        F = F ./ maximum(F, dims=nd)                                                     # :104
    end
    (w=w, v=vg, F=F, P=P, FBl=FBl, FBu=FBu, FBm=FBm, PBl=PBl, PBu=PBu, PBm=PBm, line=(mcmean && FBm !== nothing) ? FBm : F)
end

# ---- spectrogram / melspectrogram / mfcc: DSP.spectrogram + src/mel.jl (STFT, mel bands and MFCC on the device) ----------------
# The filterbank and the DCT come from the library (host C, the reference's precision); the STFT and its epilogues run on the device.
struct Spectrogram{T,F,Ti}
    power::Matrix{T}
    freq::F
    time::Ti
end
struct MelSpectrogram{T,F,Ti}
    power::Matrix{T}
    mels::F
    time::Ti
end
struct MFCC{T,F,Ti}
    mfcc::Matrix{T}
    number::F
    time::Ti
end
freq(S::Spectrogram) = S.freq
freq(M::MelSpectrogram) = M.mels
freq(M::MFCC) = M.number
Base.time(S::Spectrogram) = S.time
Base.time(M::MelSpectrogram) = M.time
Base.time(M::MFCC) = M.time

function _nextfastfft(n::Integer)
    out = Ref{Int64}(0)
    check(@ccall LIB.lpvs_nextfastfft(Int64(n)::Int64, out::Ref{Int64})::Int32)
    Int(out[])
end

_hz_to_mel(f) = (m = f / (200f0 / 3); f >= 1000f0 ? (1000f0 / (200f0 / 3)) + log(f / 1000f0) / (log(6.4f0) / 27f0) : m)   # src/mel.jl:38-53

function mel(fs::Real, nfft::Int; nmels::Int = 128, fmin::Real = 0f0, fmax::Real = fs/2f0)             # src/mel.jl:99-113
    W = Matrix{Float32}(undef, nmels, (nfft >> 1) + 1)
    wide = Int32((fs isa Float64 ? 1 : 0) | (fmin isa Float64 ? 2 : 0) | (fmax isa Float64 ? 4 : 0))
    GC.@preserve W check(@ccall LIB.lpvs_mel_filterbank(Float64(fs)::Float64, Int64(nfft)::Int64, Int64(nmels)::Int64, Float64(fmin)::Float64,
        Float64(fmax)::Float64, wide::Int32, W::Ptr{Float32})::Int32)
    W
end

function dct_matrix(nfilters::Int, ninput::Int)                                                       # src/mel.jl dct_matrix
    D = Matrix{Float32}(undef, nfilters, ninput)
    GC.@preserve D check(@ccall LIB.lpvs_dct_matrix(Int64(nfilters)::Int64, Int64(ninput)::Int64, D::Ptr{Float32})::Int32)
    D
end

# one STFT call: kind 1 power, 2 mel bands (W), 3 MFCC (W, D); Float32 signals take the _f32 entry point
function _stft(kind::Int32, s::AbstractVector{<:Real}, n::Integer, noverlap::Integer, nfft::Integer, fs::Real, window, W, D; device::Integer=0)
    nbins = nfft ÷ 2 + 1
    rows = kind == 1 ? nbins : (kind == 2 ? size(W, 1) : size(D, 1))
    Wv = W === nothing ? Float32[] : Matrix{Float32}(W)
    Dv = D === nothing ? Float32[] : Matrix{Float32}(D)
    nmels = Int64(W === nothing ? 0 : size(W, 1)); nmfcc = Int64(D === nothing ? 0 : size(D, 1))
    k = Ref{Int64}(0)
    if eltype(s) == Float32
        sv = Vector{Float32}(s)
        wv = window === nothing ? Float32[] : Vector{Float32}(window isa Function ? window(n) : window)
        wp = window === nothing ? Ptr{Float32}(C_NULL) : pointer(wv)
        GC.@preserve sv wv Wv Dv check(@ccall LIB.lpvs_stft_f32(kind::Int32, sv::Ptr{Float32}, Int64(length(sv))::Int64, Int64(n)::Int64,
            Int64(noverlap)::Int64, Int64(nfft)::Int64, Float64(fs)::Float64, wp::Ptr{Float32}, Wv::Ptr{Float32}, nmels::Int64, Dv::Ptr{Float32},
            nmfcc::Int64, Int32(device)::Int32, C_NULL::Ptr{Float32}, Int64(0)::Int64, k::Ref{Int64})::Int32)
        out = Matrix{Float32}(undef, rows, k[])
        GC.@preserve sv wv Wv Dv out check(@ccall LIB.lpvs_stft_f32(kind::Int32, sv::Ptr{Float32}, Int64(length(sv))::Int64, Int64(n)::Int64,
            Int64(noverlap)::Int64, Int64(nfft)::Int64, Float64(fs)::Float64, wp::Ptr{Float32}, Wv::Ptr{Float32}, nmels::Int64, Dv::Ptr{Float32},
            nmfcc::Int64, Int32(device)::Int32, out::Ptr{Float32}, Int64(length(out))::Int64, k::Ref{Int64})::Int32)
    else
        sv = Vector{Float64}(s)
        wv = window === nothing ? Float64[] : Vector{Float64}(window isa Function ? window(n) : window)
        wp = window === nothing ? Ptr{Float64}(C_NULL) : pointer(wv)
        GC.@preserve sv wv Wv Dv check(@ccall LIB.lpvs_stft_f64(kind::Int32, sv::Ptr{Float64}, Int64(length(sv))::Int64, Int64(n)::Int64,
            Int64(noverlap)::Int64, Int64(nfft)::Int64, Float64(fs)::Float64, wp::Ptr{Float64}, Wv::Ptr{Float32}, nmels::Int64, Dv::Ptr{Float32},
            nmfcc::Int64, Int32(device)::Int32, C_NULL::Ptr{Float64}, Int64(0)::Int64, k::Ref{Int64})::Int32)
        out = Matrix{Float64}(undef, rows, k[])
        GC.@preserve sv wv Wv Dv out check(@ccall LIB.lpvs_stft_f64(kind::Int32, sv::Ptr{Float64}, Int64(length(sv))::Int64, Int64(n)::Int64,
            Int64(noverlap)::Int64, Int64(nfft)::Int64, Float64(fs)::Float64, wp::Ptr{Float64}, Wv::Ptr{Float32}, nmels::Int64, Dv::Ptr{Float32},
            nmfcc::Int64, Int32(device)::Int32, out::Ptr{Float64}, Int64(length(out))::Int64, k::Ref{Int64})::Int32)
    end
    out, ((0:k[]-1) .* (n - noverlap) .+ n / 2) ./ fs
end

function spectrogram(s::AbstractVector{<:Real}, n::Int = length(s) >> 3, noverlap::Int = n >> 1; nfft::Int = _nextfastfft(n), fs::Real = 1,
                     window = nothing, device::Integer = 0)                                             # DSP.spectrogram (real s)
    P, t = _stft(Int32(1), s, n, noverlap, nfft, fs, window, nothing, nothing; device=device)
    Spectrogram(P, (0:nfft÷2) .* (fs / nfft), t)
end

function melspectrogram(S::Spectrogram; fs=1, nmels::Int = 128, fmin::Real = 0f0, fmax::Real = fs / 2f0, device::Integer = 0)   # src/mel.jl:133-138
    nbins, frames = size(S.power)
    W = mel(fs, 2nbins - 1; nmels=nmels, fmin=fmin, fmax=fmax)
    if eltype(S.power) == Float32
        P32 = Matrix{Float32}(S.power); out32 = Matrix{Float32}(undef, nmels, frames)
        GC.@preserve P32 W out32 check(@ccall LIB.lpvs_mel_project_f32(P32::Ptr{Float32}, Int64(nbins)::Int64, Int64(frames)::Int64, W::Ptr{Float32},
            Int64(nmels)::Int64, Int32(device)::Int32, out32::Ptr{Float32})::Int32)
        return MelSpectrogram(out32, LinRange(_hz_to_mel(fmin), _hz_to_mel(fmax), nmels), S.time)
    end
    P64 = Matrix{Float64}(S.power); out64 = Matrix{Float64}(undef, nmels, frames)
    GC.@preserve P64 W out64 check(@ccall LIB.lpvs_mel_project_f64(P64::Ptr{Float64}, Int64(nbins)::Int64, Int64(frames)::Int64, W::Ptr{Float32},
        Int64(nmels)::Int64, Int32(device)::Int32, out64::Ptr{Float64})::Int32)
    MelSpectrogram(out64, LinRange(_hz_to_mel(fmin), _hz_to_mel(fmax), nmels), S.time)
end

function melspectrogram(s, n=div(length(s), 8), args...; fs=1, nmels::Int = 128, fmin::Real = 0f0, fmax::Real = fs / 2f0, window=hanning,
                        kwargs...)                                                                    # src/mel.jl:140-143, fused on the device
    noverlap = isempty(args) ? get(kwargs, :noverlap, n >> 1) : args[1]
    nfft = get(kwargs, :nfft, _nextfastfft(n))
    device = get(kwargs, :device, 0)
    W = mel(fs, 2(nfft ÷ 2 + 1) - 1; nmels=nmels, fmin=fmin, fmax=fmax)
    P, t = _stft(Int32(2), s, n, noverlap, nfft, fs, window, W, nothing; device=device)
    MelSpectrogram(P, LinRange(_hz_to_mel(fmin), _hz_to_mel(fmax), nmels), t)
end

function mfcc(s, args...; nmfcc::Int = 20, nmels::Int = 128, window=hanning, kwargs...)             # src/mel.jl:159-172
    if nmfcc >= nmels
        error("number of mfcc components should be less than the number of mel frequency bins")
    end
    n = isempty(args) ? div(length(s), 8) : args[1]
    noverlap = length(args) > 1 ? args[2] : get(kwargs, :noverlap, n >> 1)
    nfft = get(kwargs, :nfft, _nextfastfft(n)); fs = get(kwargs, :fs, 1)
    fmin = get(kwargs, :fmin, 0f0); fmax = get(kwargs, :fmax, fs / 2f0); device = get(kwargs, :device, 0)
    W = mel(fs, 2(nfft ÷ 2 + 1) - 1; nmels=nmels, fmin=fmin, fmax=fmax)
    C, t = _stft(Int32(3), s, n, noverlap, nfft, fs, window, W, dct_matrix(nmfcc, nmels); device=device)
    MFCC(C, 1:nmfcc, t)
end

# ---- welch_pgram / periodogram (DSP.jl) and the numbers of the heat-map recipes (src/plotting.jl:15-47) -------------------------------
# The frame average is summed on the device without the power matrix; compress selects its order statistics by an exact radix select.
struct Periodogram{T,F}
    power::Vector{T}
    freq::F
end
freq(P::Periodogram) = P.freq

function _welch(s::AbstractVector{<:Real}, n::Integer, noverlap::Integer, nfft::Integer, fs::Real, window, onesided::Bool; device::Integer=0)
    rows = onesided ? nfft ÷ 2 + 1 : nfft
    k = Ref{Int64}(0)
    if eltype(s) == Float32
        sv = Vector{Float32}(s)
        wv = window === nothing ? Float32[] : Vector{Float32}(window isa Function ? window(n) : window)
        wp = window === nothing ? Ptr{Float32}(C_NULL) : pointer(wv)
        out = Vector{Float32}(undef, rows)
        GC.@preserve sv wv out check(@ccall LIB.lpvs_welch_f32(sv::Ptr{Float32}, Int64(length(sv))::Int64, Int64(n)::Int64, Int64(noverlap)::Int64,
            Int64(nfft)::Int64, Float64(fs)::Float64, wp::Ptr{Float32}, Int32(onesided)::Int32, Int32(device)::Int32, out::Ptr{Float32},
            k::Ref{Int64})::Int32)
    else
        sv = Vector{Float64}(s)
        wv = window === nothing ? Float64[] : Vector{Float64}(window isa Function ? window(n) : window)
        wp = window === nothing ? Ptr{Float64}(C_NULL) : pointer(wv)
        out = Vector{Float64}(undef, rows)
        GC.@preserve sv wv out check(@ccall LIB.lpvs_welch_f64(sv::Ptr{Float64}, Int64(length(sv))::Int64, Int64(n)::Int64, Int64(noverlap)::Int64,
            Int64(nfft)::Int64, Float64(fs)::Float64, wp::Ptr{Float64}, Int32(onesided)::Int32, Int32(device)::Int32, out::Ptr{Float64},
            k::Ref{Int64})::Int32)
    end
    f = onesided ? (0:nfft÷2) .* (fs / nfft) : [(j <= (nfft - 1) ÷ 2 ? j : j - nfft) * (fs / nfft) for j in 0:nfft-1]
    Periodogram(out, f)
end

function welch_pgram(s::AbstractVector{<:Real}, n::Int = length(s) >> 3, noverlap::Int = n >> 1; onesided::Bool = true, nfft::Int = _nextfastfft(n),
                     fs::Real = 1, window = nothing, device::Integer = 0)                                 # DSP.welch_pgram (real s)
    _welch(s, n, noverlap, nfft, fs, window, onesided; device=device)
end

function periodogram(s::AbstractVector{<:Real}; onesided::Bool = true, nfft::Int = _nextfastfft(length(s)), fs::Real = 1, window = nothing,
                     device::Integer = 0)                                                                 # DSP.periodogram (real s)
    _welch(s, length(s), 0, nfft, fs, window, onesided; device=device)
end

# ---- generalised Lomb-Scargle periodogram (extension: the non-uniform twin of periodogram; include/lpvspectral.h g4) ----------------
const LOMB_NORMALIZATIONS = Dict(:standard => Int32(0), :psd => Int32(1))
"""    lombscargle(y, t, f=default_freqs(t); W=nothing, fit_mean=true, center_data=true, normalization=:standard, path=:auto, coef=false, nterms=1)
Every frequency fitted on its own, `y ≈ c + a cos 2πft + b sin 2πft` in weighted least squares; `y` a vector or an N × ns matrix of
signals sharing `t`.  Returns `(power = Nf or Nf × ns, freq = f)` and, with `coef=true`, also `(a, b, c)`.
`nterms = K` in 2:6 fits K harmonics per frequency, `y ≈ c + Σ_h a_h cos 2πhft + b_h sin 2πhft` (include/lpvspectral.h g7; direct sums
only: `path=:nufft` is an ArgumentError); `a`, `b` are then Nf × K (one signal) or Nf × ns × K, `c` as before."""
function lombscargle(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}=default_freqs(t); W=nothing, fit_mean::Bool=true,
                     center_data::Bool=true, normalization::Symbol=:standard, path::Symbol=:auto, device::Integer=0, coef::Bool=false, nterms::Integer=1)
    tv, fv = Vector{Float64}(t), Vector{Float64}(f)
    N, Nf, ns = length(tv), length(fv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    power = zeros(Nf, ns)
    1 <= nterms <= 6 || throw(ArgumentError("nterms must be in 1:6, got $nterms"))
    if nterms > 1
        haskey(EVAL_PATHS, path) || throw(ArgumentError("path: unknown value $path"))
        path == :nufft && throw(ArgumentError("path=:nufft: the transforms are not implemented for several terms (nterms = $nterms)"))
        K = Int(nterms)
        ctv = coef ? zeros(Nf, ns, 2K + 1) : Float64[]                       # planes a_1, b_1, a_2, ..., then c
        ctp = coef ? pointer(ctv) : Ptr{Float64}(C_NULL)
        GC.@preserve yv tv Wv fv power ctv check(@ccall LIB.lpvs_lombscargle_terms_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64}, Int64(N)::Int64,
            Wp::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, Int32(K)::Int32, Int32(fit_mean)::Int32, Int32(center_data)::Int32,
            LOMB_NORMALIZATIONS[normalization]::Int32, Int32(device)::Int32, power::Ptr{Float64}, ctp::Ptr{Float64}, C_NULL::Ptr{Float64})::Int32)
        shapedk(A) = y isa AbstractVector ? reshape(A, Nf, :) : A
        Pk = (power = y isa AbstractVector ? vec(power) : power, freq = fv)
        return coef ? (Pk, (shapedk(ctv[:, :, 1:2:2K]), shapedk(ctv[:, :, 2:2:2K]), y isa AbstractVector ? vec(ctv[:, :, 2K + 1]) : ctv[:, :, 2K + 1])) : Pk
    end
    cfv = coef ? zeros(Nf, ns, 3) : Float64[]
    cfp = coef ? pointer(cfv) : Ptr{Float64}(C_NULL)
    GC.@preserve yv tv Wv fv power cfv check(@ccall LIB.lpvs_lombscargle_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64}, Int64(N)::Int64, Wp::Ptr{Float64},
        fv::Ptr{Float64}, Int64(Nf)::Int64, Int32(fit_mean)::Int32, Int32(center_data)::Int32, LOMB_NORMALIZATIONS[normalization]::Int32, EVAL_PATHS[path]::Int32,
        Int32(device)::Int32, power::Ptr{Float64}, cfp::Ptr{Float64}, C_NULL::Ptr{Float64})::Int32)
    shaped(A) = y isa AbstractVector ? vec(A) : A
    P = (power = shaped(power), freq = fv)
    coef ? (P, (shaped(cfv[:, :, 1]), shaped(cfv[:, :, 2]), shaped(cfv[:, :, 3]))) : P
end
function lombscargle_terms_last_timing()
    tm = zeros(10)
    GC.@preserve tm check(@ccall LIB.lpvs_lombscargle_terms_last_timing(tm::Ptr{Float64}, Int32(10)::Int32)::Int32)
    (nterms=Int(tm[1]), ts=Int(tm[2]), slabs=Int(tm[3]), degenerate=Int(tm[4]), moments_ms=tm[5], sums_ms=tm[6], epilogue_ms=tm[7], copy_ms=tm[8], total_ms=tm[9],
     accumulators=Int(tm[10]))
end
function lombscargle_last_timing()
    tm = zeros(12)
    GC.@preserve tm check(@ccall LIB.lpvs_lombscargle_last_timing(tm::Ptr{Float64}, Int32(12)::Int32)::Int32)
    (path=Int(tm[1]), blocks=(Int(tm[2]), Int(tm[3])), nf=Int(tm[4]), degenerate=Int(tm[5]), slabs=Int(tm[6]), moments_ms=tm[7], sums_ms=tm[8], epilogue_ms=tm[9],
     copy_ms=tm[10], total_ms=tm[11], twin=tm[12] != 0)
end

# ---- windowed Lomb-Scargle (extension: the non-uniform twins of spectrogram and welch_pgram; include/lpvspectral.h g5) -----------------
const LOMB_TAPERS = Dict(:rect => Int32(0), :hanning => Int32(1))
"""    time_windows(t, lo, hi) -> (starts, counts)
0-based index ranges of the time intervals `[lo[w], hi[w]]` in a non-decreasing `t`: one binary search per edge on the device."""
function time_windows(t::AbstractVector{<:Real}, lo::AbstractVector{<:Real}, hi::AbstractVector{<:Real}; device::Integer=0)
    tv, lov, hiv = Vector{Float64}(t), Vector{Float64}(lo), Vector{Float64}(hi)
    @assert length(lov) == length(hiv) "lo and hi have to be the same length"
    starts, counts = zeros(Int64, length(lov)), zeros(Int64, length(lov))
    GC.@preserve tv lov hiv starts counts check(@ccall LIB.lpvs_time_windows_f64(tv::Ptr{Float64}, Int64(length(tv))::Int64, lov::Ptr{Float64}, hiv::Ptr{Float64},
        Int64(length(lov))::Int64, Int32(device)::Int32, starts::Ptr{Int64}, counts::Ptr{Int64})::Int32)
    starts, counts
end
# (starts 0-based, counts, lo, hi) of the one window form that was given
function _lomb_window_list(t::Vector{Float64}, n, noverlap, width, hop, windows, device)
    forms = (n !== nothing || noverlap !== nothing) + (width !== nothing || hop !== nothing) + (windows !== nothing)
    forms > 1 && throw(ArgumentError("give the windows in one form: n (noverlap), width (hop) or windows=(starts, counts, lo, hi)"))
    if windows !== nothing
        return Vector{Int64}(windows[1]), Vector{Int64}(windows[2]), Vector{Float64}(windows[3]), Vector{Float64}(windows[4])
    elseif width !== nothing || hop !== nothing
        width === nothing && throw(ArgumentError("hop needs width"))
        h = hop === nothing ? width / 2 : hop
        lo = Float64[]
        while t[1] + length(lo) * h <= t[end]
            push!(lo, t[1] + length(lo) * h)
        end
        hi = lo .+ Float64(width)
        starts, counts = time_windows(t, lo, hi; device=device)
        return starts, counts, lo, hi
    end
    nn = n === nothing ? length(t) >> 3 : Int(n)
    nov = noverlap === nothing ? nn >> 1 : Int(noverlap)
    starts = Vector{Int64}(_offsets(length(t), nn, nov))                      # (0-based, as the library counts)
    starts, fill(Int64(nn), length(starts)), t[starts .+ 1], t[starts .+ nn]
end
function _lomb_windows(y, t, f, n, noverlap, width, hop, windows, window, W, fit_mean, center_data, normalization, coef, average, device)
    tv, fv = Vector{Float64}(t), Vector{Float64}(f)
    N, Nf, ns = length(tv), length(fv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    taper = window === hanning ? LOMB_TAPERS[:hanning] : window === rect ? LOMB_TAPERS[:rect] : throw(ArgumentError("window: hanning or rect"))
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    starts, counts, lov, hiv = _lomb_window_list(tv, n, noverlap, width, hop, windows, device)
    nwin = length(starts)
    power = average ? zeros(Nf, ns) : zeros(Nf, nwin, ns)
    cfv = coef ? zeros(Nf, nwin, ns, 3) : Float64[]
    cfp = coef ? pointer(cfv) : Ptr{Float64}(C_NULL)
    empty = zeros(Int32, nwin)
    GC.@preserve yv tv Wv fv starts counts lov hiv power cfv empty check(@ccall LIB.lpvs_lombscargle_windows_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64},
        Int64(N)::Int64, Wp::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, starts::Ptr{Int64}, counts::Ptr{Int64}, lov::Ptr{Float64}, hiv::Ptr{Float64},
        Int64(nwin)::Int64, taper::Int32, Int32(fit_mean)::Int32, Int32(center_data)::Int32, LOMB_NORMALIZATIONS[normalization]::Int32, Int32(average)::Int32,
        Int32(device)::Int32, power::Ptr{Float64}, cfp::Ptr{Float64}, empty::Ptr{Int32})::Int32)
    one = y isa AbstractVector
    average && return (power = one ? vec(power) : power, freq = fv)
    shaped(A) = one ? A[:, :, 1] : A
    S = (power = shaped(power), freq = fv, time = (lov .+ hiv) ./ 2, counts = counts, empty = empty .!= 0)
    coef ? (S, (shaped(cfv[:, :, :, 1]), shaped(cfv[:, :, :, 2]), shaped(cfv[:, :, :, 3]))) : S
end
"""    lombscargle_spectrogram(y, t, f=default_freqs(t); n, noverlap, width, hop, windows, window=hanning, W, fit_mean, center_data, normalization, coef)
The `lombscargle` estimate of every window of the record in one batched call; the windows in ONE of the forms `n` (`noverlap`), `width`
(`hop`) or `windows=(starts, counts, lo, hi)` (0-based starts).  The taper is evaluated from the sample times.  Returns
`(power = Nf × nwin (× ns), freq, time, counts, empty)` and, with `coef=true`, also `(a, b, c)`."""
function lombscargle_spectrogram(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}=default_freqs(t); n=nothing, noverlap=nothing,
                                 width=nothing, hop=nothing, windows=nothing, window=hanning, W=nothing, fit_mean::Bool=true, center_data::Bool=true,
                                 normalization::Symbol=:standard, coef::Bool=false, device::Integer=0)
    _lomb_windows(y, t, f, n, noverlap, width, hop, windows, window, W, fit_mean, center_data, normalization, coef, false, device)
end
"""    lombscargle_welch(y, t, f=default_freqs(t); ...) -> (power, freq)
The mean of the columns of `lombscargle_spectrogram` over the windows that are not empty, added on the device in a fixed order."""
function lombscargle_welch(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}=default_freqs(t); n=nothing, noverlap=nothing,
                           width=nothing, hop=nothing, windows=nothing, window=hanning, W=nothing, fit_mean::Bool=true, center_data::Bool=true,
                           normalization::Symbol=:standard, device::Integer=0)
    _lomb_windows(y, t, f, n, noverlap, width, hop, windows, window, W, fit_mean, center_data, normalization, false, true, device)
end
function lombscargle_windows_last_timing()
    tm = zeros(10)
    GC.@preserve tm check(@ccall LIB.lpvs_lombscargle_windows_last_timing(tm::Ptr{Float64}, Int32(10)::Int32)::Int32)
    (windows=Int(tm[1]), empty=Int(tm[2]), items=Int(tm[3]), slab=Int(tm[4]), degenerate=Int(tm[5]), moments_ms=tm[6], sums_ms=tm[7], epilogue_ms=tm[8],
     copy_ms=tm[9], total_ms=tm[10])
end

# ---- weighted wavelet Z-transform (extension; include/lpvspectral.h g8) -----------------------------------------------------------------
const WWZ_DECAY = 1 / (8 * pi^2)
"""    wwz_radius(f, c=1/(8π²), wmin=1e-9)
How far a cell of `wwz` reaches: `sqrt(log(1 / wmin) / c) / (2π f)`, `Inf` for `wmin = 0`."""
wwz_radius(f::AbstractVector{<:Real}, c::Real=WWZ_DECAY, wmin::Real=1e-9) =
    wmin == 0 ? fill(Inf, length(f)) : sqrt(log(1 / Float64(wmin)) / Float64(c)) ./ (2 * pi .* Vector{Float64}(f))
"""    wwz(y, t, f=default_freqs(t)[2:end]; tau=nothing, ntau=nothing, c=1/(8π²), wmin=1e-9, W=nothing, center_data=true, coef=false)
Foster's weighted wavelet Z-transform of non-uniformly sampled signals: at every time `tau[j]` and frequency `f[k]` the floating-mean fit
of `lombscargle` under the weights `W exp(-c (2π f (t - tau))²)`.  `t` non-decreasing; `tau` defaults to `ntau` (64) equally spaced times
over the record.  Returns `(power, wwz, amplitude = Nf × Ntau (× ns), neff, counts, empty = Nf × Ntau, freq, time, radius)` and, with
`coef=true`, also `(a, b, c)` (phase origin `t = 0`)."""
function wwz(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}=default_freqs(t)[2:end]; tau=nothing, ntau=nothing,
             c::Real=WWZ_DECAY, wmin::Real=1e-9, W=nothing, center_data::Bool=true, coef::Bool=false, device::Integer=0)
    tv, fv = Vector{Float64}(t), Vector{Float64}(f)
    tau !== nothing && ntau !== nothing && throw(ArgumentError("give tau or ntau, not both"))
    tauv = tau === nothing ? collect(range(tv[1], tv[end]; length=(ntau === nothing ? 64 : Int(ntau)))) : Vector{Float64}(tau)
    N, Nf, Ntau, ns = length(tv), length(fv), length(tauv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    radius = wwz_radius(fv, c, wmin)
    power, amplitude, z, neff = zeros(Nf, Ntau, ns), zeros(Nf, Ntau, ns), zeros(Nf, Ntau, ns), zeros(Nf, Ntau)
    cfv = coef ? zeros(Nf, Ntau, ns, 3) : Float64[]
    cfp = coef ? pointer(cfv) : Ptr{Float64}(C_NULL)
    counts, empty = zeros(Int64, Nf, Ntau), zeros(Int32, Nf, Ntau)
    GC.@preserve yv tv Wv fv tauv radius power amplitude z neff cfv counts empty check(@ccall LIB.lpvs_wwz_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64},
        Int64(N)::Int64, Wp::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, tauv::Ptr{Float64}, Int64(Ntau)::Int64, Float64(c)::Float64, radius::Ptr{Float64},
        Int32(center_data)::Int32, Int32(device)::Int32, power::Ptr{Float64}, amplitude::Ptr{Float64}, z::Ptr{Float64}, neff::Ptr{Float64}, cfp::Ptr{Float64},
        counts::Ptr{Int64}, empty::Ptr{Int32})::Int32)
    one = y isa AbstractVector
    shaped(A) = one ? A[:, :, 1] : A
    R = (power = shaped(power), wwz = shaped(z), amplitude = shaped(amplitude), neff = neff, counts = counts, empty = empty .!= 0, freq = fv, time = tauv,
         radius = radius)
    coef ? (R, (shaped(cfv[:, :, :, 1]), shaped(cfv[:, :, :, 2]), shaped(cfv[:, :, :, 3]))) : R
end
function wwz_last_timing()
    tm = zeros(16)
    GC.@preserve tm check(@ccall LIB.lpvs_wwz_last_timing(tm::Ptr{Float64}, Int32(16)::Int32)::Int32)
    (nf=Int(tm[1]), ntau=Int(tm[2]), tt=Int(tm[3]), ts=Int(tm[4]), items=Int(tm[5]), slab=Int(tm[6]), empty=Int(tm[7]), degenerate=Int(tm[8]), staged=tm[9],
     useful=tm[10], scan_ms=tm[11], ranges_ms=tm[12], sums_ms=tm[13], epilogue_ms=tm[14], copy_ms=tm[15], total_ms=tm[16])
end

# ---- box least squares periodogram (extension; include/lpvspectral.h g9) ---------------------------------------------------------------
"""    bls_frequencies(t, fmin, fmax, qmin; oversample=3)
The frequency grid of a box search: from `fmin` up to `fmax` in steps of `qmin / (oversample (max t - min t))`."""
function bls_frequencies(t::AbstractVector{<:Real}, fmin::Real, fmax::Real, qmin::Real; oversample::Real=3)
    span = Float64(maximum(t) - minimum(t))
    (span > 0 && qmin > 0 && oversample > 0 && 0 < fmin <= fmax) || throw(ArgumentError("bls_frequencies: need max t > min t, qmin > 0, oversample > 0 and 0 < fmin <= fmax"))
    df = Float64(qmin) / (Float64(oversample) * span)
    Float64(fmin) .+ df .* (0:floor(Int, (Float64(fmax) - Float64(fmin)) / df))
end
"""    bls(y, t, f; W=nothing, nbins=200, q=(0.01, 0.1), duration=nothing, min_count=1, dips_only=true, center_data=true, normalization=:standard, return_hist=false)
Box least squares periodogram (Kovács, Zucker & Mazeh 2002, binned) of non-uniformly sampled signals: at every frequency the record is
folded into `nbins` phase bins and every box of adjacent bins (wrapping) is tried as a two-level model.  `q = (qmin, qmax)` gives the
widths `max(1, floor(qmin nbins)) .. min(nbins ÷ 2, ceil(qmax nbins))` bins, `duration = (dmin, dmax)` in units of `t` the same per
frequency with `q = d f`.  `normalization`: `:standard` (share of the weighted variance, in [0, 1]) or `:chi2` (`snr²`).  Returns
`(freq, power, depth, depth_err, snr, start, width, q, duration, transit_time, count_in, degenerate)` (`start` 0-based, as the phase
`start / nbins`), each `Nf` (`× ns`), and with `return_hist=true` also `hist` (`nbins × (1 + ns) × Nf` Int64) and `hcount` (`nbins × Nf`)."""
function bls(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}; W=nothing, nbins::Integer=200, q=(0.01, 0.1), duration=nothing,
             min_count::Integer=1, dips_only::Bool=true, center_data::Bool=true, normalization::Symbol=:standard, device::Integer=0, return_hist::Bool=false)
    normalization in (:standard, :chi2) || throw(ArgumentError("normalization: unknown value $normalization (known: :standard, :chi2)"))
    tv, fv = Vector{Float64}(t), Vector{Float64}(f)
    N, Nf, ns = length(tv), length(fv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    qlo = duration === nothing ? fill(Float64(q[1]), Nf) : Float64(duration[1]) .* fv
    qhi = duration === nothing ? fill(Float64(q[2]), Nf) : Float64(duration[2]) .* fv
    clampk(x) = isfinite(x) ? Int32(clamp(x, 0, 2.0^30)) : Int32(0)
    kmin = clampk.(max.(1.0, floor.(qlo .* nbins)))
    kmax = clampk.(min.(Float64(nbins ÷ 2), ceil.(qhi .* nbins)))
    power, depth, depth_err = zeros(Nf, ns), zeros(Nf, ns), zeros(Nf, ns)
    start, width, degenerate, count_in = zeros(Int32, Nf, ns), zeros(Int32, Nf, ns), zeros(Int32, Nf, ns), zeros(Int64, Nf, ns)
    histv = return_hist ? zeros(Int64, max(nbins, 0), 1 + ns, Nf) : Int64[]
    hcountv = return_hist ? zeros(Int32, max(nbins, 0), Nf) : Int32[]
    histp = return_hist ? pointer(histv) : Ptr{Int64}(C_NULL)
    hcountp = return_hist ? pointer(hcountv) : Ptr{Int32}(C_NULL)
    GC.@preserve yv tv Wv fv kmin kmax power depth depth_err start width count_in degenerate histv hcountv check(@ccall LIB.lpvs_bls_f64(yv::Ptr{Float64},
        Int64(ns)::Int64, tv::Ptr{Float64}, Int64(N)::Int64, Wp::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, Int32(nbins)::Int32, kmin::Ptr{Int32},
        kmax::Ptr{Int32}, Int64(min_count)::Int64, Int32(dips_only)::Int32, Int32(center_data)::Int32, Int32(normalization == :chi2 ? 1 : 0)::Int32,
        Int32(device)::Int32, power::Ptr{Float64}, depth::Ptr{Float64}, depth_err::Ptr{Float64}, start::Ptr{Int32}, width::Ptr{Int32}, count_in::Ptr{Int64},
        degenerate::Ptr{Int32}, histp::Ptr{Int64}, hcountp::Ptr{Int32})::Int32)
    one = y isa AbstractVector
    shaped(A) = one ? A[:, 1] : A
    snr = map((d, e) -> e > 0 ? d / e : 0.0, depth, depth_err)
    qq = width ./ Float64(nbins)
    R = (freq = fv, power = shaped(power), depth = shaped(depth), depth_err = shaped(depth_err), snr = shaped(snr), start = shaped(start), width = shaped(width),
         q = shaped(qq), duration = shaped(qq ./ fv), transit_time = shaped((start .+ width ./ 2) ./ Float64(nbins) ./ fv), count_in = shaped(count_in),
         degenerate = shaped(degenerate .!= 0))
    return_hist ? merge(R, (hist = histv, hcount = hcountv)) : R
end
function bls_last_timing()
    tm = zeros(16)
    GC.@preserve tm check(@ccall LIB.lpvs_bls_last_timing(tm::Ptr{Float64}, Int32(16)::Int32)::Int32)
    (F=Int(tm[1]), ts=Int(tm[2]), passes=Int(tm[3]), lds_bytes=Int(tm[4]), shift_w=Int(tm[5]), shift_y_min=Int(tm[6]), shift_y_max=Int(tm[7]), degenerate=Int(tm[8]),
     boxes=tm[9], unit=tm[10] != 0, scan_ms=tm[11], quantise_ms=tm[12], search_ms=tm[13], copy_ms=tm[14], total_ms=tm[15], nf=Int(tm[16]))
end

# ---- fold statistics: pdm, aov, conditional_entropy (extension; include/lpvspectral.h g10) ----------------------------------------------
"""    pdm(y, t, f; W=nothing, nbins=10, covers=1, center_data=true, return_hist=false)
Phase dispersion minimisation (Stellingwerf 1978) with the bin covers `(Nb, Nc) = (nbins, covers)`: the record is folded into
`nbins covers` fine bins, a coarse bin is `covers` adjacent fine bins (wrapping) and every cover is used.  Returns
`(f, theta, aov, explained, nonempty, degenerate, nbins, covers)`: `explained` the share of the weighted variance between the bins,
`nonempty = M` the coarse bins that hold weight, `theta = (1 - explained) covers (N - 1) / (covers N - M)` (small at a period; 1 where
degenerate) and, for `covers = 1`, `aov = explained / (1 - explained) (N - M) / (M - 1)` (`nothing` otherwise; 0 where degenerate);
with `return_hist=true` also `hist` (`nfine × (1 + ns) × Nf` Int64) and `hcount` (`nfine × Nf`)."""
function pdm(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}; W=nothing, nbins::Integer=10, covers::Integer=1,
             center_data::Bool=true, device::Integer=0, return_hist::Bool=false)
    tv, fv = Vector{Float64}(t), Vector{Float64}(f)
    N, Nf, ns = length(tv), length(fv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    nfine = (0 < nbins <= 2048 && 0 < covers <= 2048) ? Int(nbins) * Int(covers) : 0
    explained, nonempty, degenerate = zeros(Nf, ns), zeros(Int32, Nf), zeros(Int32, Nf, ns)
    histv = return_hist ? zeros(Int64, nfine, 1 + ns, Nf) : Int64[]
    hcountv = return_hist ? zeros(Int32, nfine, Nf) : Int32[]
    histp = return_hist ? pointer(histv) : Ptr{Int64}(C_NULL)
    hcountp = return_hist ? pointer(hcountv) : Ptr{Int32}(C_NULL)
    GC.@preserve yv tv Wv fv explained nonempty degenerate histv hcountv check(@ccall LIB.lpvs_pdm_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64},
        Int64(N)::Int64, Wp::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, Int32(nbins)::Int32, Int32(covers)::Int32, Int32(center_data)::Int32,
        Int32(device)::Int32, explained::Ptr{Float64}, nonempty::Ptr{Int32}, degenerate::Ptr{Int32}, histp::Ptr{Int64}, hcountp::Ptr{Int32})::Int32)
    deg = degenerate .!= 0
    M = Float64.(nonempty)
    theta = ifelse.(deg, 1.0, (1.0 .- explained) .* (covers * (N - 1.0)) ./ (covers * Float64(N) .- M))
    F = covers == 1 ? ifelse.(deg, 0.0, ifelse.(explained .< 1.0, explained ./ (1.0 .- explained) .* (N .- M) ./ (M .- 1.0), Inf)) : nothing
    one = y isa AbstractVector
    shaped(A) = one ? A[:, 1] : A
    R = (f = fv, theta = shaped(theta), aov = F === nothing ? nothing : shaped(F), explained = shaped(explained), nonempty = nonempty, degenerate = shaped(deg),
         nbins = Int(nbins), covers = Int(covers))
    return_hist ? merge(R, (hist = histv, hcount = hcountv)) : R
end
"""    aov(y, t, f; W=nothing, nbins=10, center_data=true, return_hist=false)
The analysis-of-variance periodogram (Schwarzenberg-Czerny 1989): `pdm` with one cover; `aov` is the between / within F ratio."""
function aov(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}; W=nothing, nbins::Integer=10, covers::Integer=1,
             center_data::Bool=true, device::Integer=0, return_hist::Bool=false)
    covers == 1 || throw(ArgumentError("aov: covers must be 1, got $covers"))
    pdm(y, t, f; W=W, nbins=nbins, covers=1, center_data=center_data, device=device, return_hist=return_hist)
end
fold_timing(tm) = (F=Int(tm[1]), ts=Int(tm[2]), passes=Int(tm[3]), lds_bytes=Int(tm[4]), copies=Int(tm[5]), shift_w=Int(tm[6]), shift_y_min=Int(tm[7]),
                   shift_y_max=Int(tm[8]), degenerate=Int(tm[9]), unit=tm[10] != 0, scan_ms=tm[11], prepare_ms=tm[12], fold_ms=tm[13], copy_ms=tm[14],
                   total_ms=tm[15], nf=Int(tm[16]))
function pdm_last_timing()
    tm = zeros(16)
    GC.@preserve tm check(@ccall LIB.lpvs_pdm_last_timing(tm::Ptr{Float64}, Int32(16)::Int32)::Int32)
    fold_timing(tm)
end
"""    conditional_entropy(y, t, f; nbins=10, mbins=5, return_hist=false)
The conditional-entropy periodogram (Graham et al. 2013): the samples are counted in `nbins` phase bins times `mbins` value bins (the
values scaled to `[min y, max y]` per signal) and `H = Σ p_ij ln(p_i / p_ij)`, in nats; the period is at the MINIMUM.  Unweighted by
definition.  Returns `(f, entropy, ylim, degenerate)` -- `entropy` `Nf` (`× ns`), `ylim` `2 × ns`, `degenerate` per signal (a constant
signal: entropy 0) -- and with `return_hist=true` also `hist` (`mbins × nbins × ns × Nf` Int32)."""
function conditional_entropy(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}; nbins::Integer=10, mbins::Integer=5,
                             device::Integer=0, return_hist::Bool=false)
    tv, fv = Vector{Float64}(t), Vector{Float64}(f)
    N, Nf, ns = length(tv), length(fv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    ok = 0 < nbins <= 256 && 0 < mbins <= 64
    entropy, ylim, degenerate = zeros(Nf, ns), zeros(2, ns), zeros(Int32, ns)
    histv = return_hist ? zeros(Int32, ok ? Int(mbins) : 0, ok ? Int(nbins) : 0, ns, Nf) : Int32[]
    histp = return_hist ? pointer(histv) : Ptr{Int32}(C_NULL)
    GC.@preserve yv tv fv entropy ylim degenerate histv check(@ccall LIB.lpvs_cent_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64}, Int64(N)::Int64,
        fv::Ptr{Float64}, Int64(Nf)::Int64, Int32(nbins)::Int32, Int32(mbins)::Int32, Int32(device)::Int32, entropy::Ptr{Float64}, ylim::Ptr{Float64},
        degenerate::Ptr{Int32}, histp::Ptr{Int32})::Int32)
    one = y isa AbstractVector
    R = (f = fv, entropy = one ? entropy[:, 1] : entropy, ylim = one ? ylim[:, 1] : ylim, degenerate = one ? degenerate[1] != 0 : degenerate .!= 0)
    return_hist ? merge(R, (hist = histv,)) : R
end
function cent_last_timing()
    tm = zeros(16)
    GC.@preserve tm check(@ccall LIB.lpvs_cent_last_timing(tm::Ptr{Float64}, Int32(16)::Int32)::Int32)
    fold_timing(tm)
end

# ---- CLEAN deconvolution: dirty_spectrum, clean_loop, clean_restore, clean (extension; include/lpvspectral.h g11) ---------------------------
const CLEAN_STATUS = (:niter, :tol, :empty)
_cplx(A::Array{Float64}) = dropdims(copy(reinterpret(ComplexF64, A)); dims=1)      # (2, ...) interleaved doubles -> complex
_ri(A::AbstractArray{<:Complex}) = Array{Float64}(reinterpret(Float64, reshape(Array{ComplexF64}(A), 1, size(A)...)))
function _clean_grid(t, df, Nf)
    df = df === nothing ? 1 / (4 * (maximum(t) - minimum(t))) : Float64(df)
    Nf = Nf === nothing ? max(2, floor(Int, default_freqs(t)[end] / df) + 1) : Int(Nf)
    df, Nf
end
"""    clean_sigma(Wn, df)
The width of the Gaussian restoring beam fitted to the spectral window: the first `m` with `|Wn_m|² < 1/2`, interpolated linearly in
`|Wn|²`, is the half width `h`; `sigma = h / sqrt(2 ln 2)` (the operations of csrc/clean_plan.h `clean_sigma`, in its order)."""
function clean_sigma(Wn::AbstractVector{<:Complex}, df::Real)
    P = real.(Wn) .* real.(Wn) .+ imag.(Wn) .* imag.(Wn)
    for m in 2:length(P)
        if P[m] < 0.5
            frac = P[m-1] > P[m] ? (P[m-1] - 0.5) / (P[m-1] - P[m]) : 0.0
            return ((Float64(m - 2) + frac) * Float64(df)) * 0.8493218002880191
        end
    end
    (Float64(length(P) - 1) * Float64(df)) * 0.8493218002880191
end
"""    dirty_spectrum(y, t; df=nothing, Nf=nothing, W=nothing, center_data=true, path=:auto)
The dirty spectrum `D_k = Σ w y_c e^{-2πi f_k t}` (`Nf` (`× ns`)) and the spectral window `Wn_m = Σ w e^{-2πi f_m t}` (`2 Nf - 1`) on the
grid `f_m = m df`: `lombscargle`'s sums by its kernels and paths.  Defaults: `df = 1 / (4 (max t - min t))`, `Nf` up to
`default_freqs(t)`'s top frequency.  Returns `(D, Wn)`."""
function dirty_spectrum(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}; df=nothing, Nf=nothing, W=nothing, center_data::Bool=true,
                        path::Symbol=:auto, device::Integer=0)
    tv = Vector{Float64}(t)
    df, Nf = _clean_grid(tv, df, Nf)
    N, ns = length(tv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    Dv, Wnv = zeros(2, max(Nf, 0), ns), zeros(2, max(2Nf - 1, 0))
    GC.@preserve yv tv Wv Dv Wnv check(@ccall LIB.lpvs_dirty_spectrum_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64}, Int64(N)::Int64, Wp::Ptr{Float64},
        Float64(df)::Float64, Int64(Nf)::Int64, Int32(center_data)::Int32, EVAL_PATHS[path]::Int32, Int32(device)::Int32, Dv::Ptr{Float64}, Wnv::Ptr{Float64})::Int32)
    D = _cplx(Dv)
    (y isa AbstractVector ? D[:, 1] : D), _cplx(Wnv)
end
"""    clean_loop(D, Wn; gain=0.5, niter=100, tol=0.0)
The CLEAN loop on spectra the caller has (`D`: `Nf` (`× ns`), `Wn`: `2 Nf - 1`), all iterations of a signal in one kernel launch.
Returns `(R, C, picks, pick_values, iterations, status)`; `picks` 1-based in the order picked, 0 behind the last (`niter` (`× ns`));
`status` `:niter`, `:tol` or `:empty`."""
function clean_loop(D::AbstractVecOrMat{<:Complex}, Wn::AbstractVector{<:Complex}; gain::Real=0.5, niter::Integer=100, tol::Real=0.0, device::Integer=0)
    Nf, ns = size(D, 1), size(D, 2)
    @assert length(Wn) == 2Nf - 1 "Wn has to hold 2 Nf - 1 values"
    Dv, Wnv = _ri(reshape(D, Nf, ns)), _ri(Wn)
    nit = max(Int(niter), 0)
    Rv, Cv, pvv = zeros(2, Nf, ns), zeros(2, Nf, ns), zeros(2, max(nit, 1), ns)
    picks, iters, status = fill(Int32(-1), max(nit, 1), ns), zeros(Int32, ns), zeros(Int32, ns)
    GC.@preserve Dv Wnv Rv Cv pvv picks iters status check(@ccall LIB.lpvs_clean_loop_f64(Dv::Ptr{Float64}, Int64(ns)::Int64, Int64(Nf)::Int64, Wnv::Ptr{Float64},
        Float64(gain)::Float64, Int64(niter)::Int64, Float64(tol)::Float64, Int32(device)::Int32, Rv::Ptr{Float64}, Cv::Ptr{Float64}, picks::Ptr{Int32},
        pvv::Ptr{Float64}, iters::Ptr{Int32}, status::Ptr{Int32})::Int32)
    one = D isa AbstractVector
    sh(A) = one ? A[:, 1] : A
    sh(_cplx(Rv)), sh(_cplx(Cv)), sh(Int.(picks[1:nit, :]) .+ 1), sh(_cplx(pvv)[1:nit, :]), one ? Int(iters[1]) : Int.(iters),
        one ? CLEAN_STATUS[status[1]+1] : [CLEAN_STATUS[v+1] for v in status]
end
"""    clean_restore(R, C, df, sigma)
`S_k = R_k + Σ_p [C_p B_{k-p} + conj(C_p) B_{k+p}]` with the real Gaussian beam `B_m = exp(-(m df)² / (2 sigma²))`."""
function clean_restore(R::AbstractVecOrMat{<:Complex}, C::AbstractVecOrMat{<:Complex}, df::Real, sigma::Real; device::Integer=0)
    Nf, ns = size(R, 1), size(R, 2)
    @assert size(C) == size(R) "C has to be shaped as R"
    Rv, Cv, Sv = _ri(reshape(R, Nf, ns)), _ri(reshape(C, Nf, ns)), zeros(2, Nf, ns)
    GC.@preserve Rv Cv Sv check(@ccall LIB.lpvs_clean_restore_f64(Rv::Ptr{Float64}, Cv::Ptr{Float64}, Int64(ns)::Int64, Int64(Nf)::Int64, Float64(df)::Float64,
        Float64(sigma)::Float64, Int32(device)::Int32, Sv::Ptr{Float64})::Int32)
    S = _cplx(Sv)
    R isa AbstractVector ? S[:, 1] : S
end
"""    clean(y, t; df=nothing, Nf=nothing, W=nothing, gain=0.5, niter=100, tol=0.0, center_data=true, center_time=true, path=:auto)
CLEAN deconvolution (Roberts, Lehár & Dreher 1987) of the spectrum of non-uniformly sampled signals: the dirty spectrum, the loop and the
restoration in one call of the library.  `center_time=true` subtracts the mean of `t` first (the beam is real: phases refer to the mean
epoch; this redefines the record by one rounding per time).  Returns `(freq, dirty, window, residual, components, picks, pick_values,
spectrum, power, amplitude, iterations, status, sigma)`; `amplitude = 2 |components|`, `picks` 1-based, 0 behind the last."""
function clean(y::AbstractVecOrMat{<:Real}, t::AbstractVector{<:Real}; df=nothing, Nf=nothing, W=nothing, gain::Real=0.5, niter::Integer=100, tol::Real=0.0,
               center_data::Bool=true, center_time::Bool=true, path::Symbol=:auto, device::Integer=0)
    tv = Vector{Float64}(t)
    df, Nf = _clean_grid(tv, df, Nf)
    center_time && (tv = tv .- sum(tv) / length(tv))
    N, ns = length(tv), size(y, 2)
    @assert size(y, 1) == N "y has to be as long as the sampling points"
    yv = Matrix{Float64}(reshape(y, N, ns))
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    nit, nf = max(Int(niter), 0), max(Nf, 0)
    Dv, Rv, Cv, Sv, Wnv, pvv = zeros(2, nf, ns), zeros(2, nf, ns), zeros(2, nf, ns), zeros(2, nf, ns), zeros(2, max(2Nf - 1, 0)), zeros(2, max(nit, 1), ns)
    picks, iters, status, sg = fill(Int32(-1), max(nit, 1), ns), zeros(Int32, ns), zeros(Int32, ns), zeros(1)
    GC.@preserve yv tv Wv Dv Wnv Rv Cv picks pvv iters status Sv sg check(@ccall LIB.lpvs_clean_f64(yv::Ptr{Float64}, Int64(ns)::Int64, tv::Ptr{Float64},
        Int64(N)::Int64, Wp::Ptr{Float64}, Float64(df)::Float64, Int64(Nf)::Int64, Int32(center_data)::Int32, EVAL_PATHS[path]::Int32, Float64(gain)::Float64,
        Int64(niter)::Int64, Float64(tol)::Float64, 0.0::Float64, Int32(device)::Int32, Dv::Ptr{Float64}, Wnv::Ptr{Float64}, Rv::Ptr{Float64}, Cv::Ptr{Float64},
        picks::Ptr{Int32}, pvv::Ptr{Float64}, iters::Ptr{Int32}, status::Ptr{Int32}, Sv::Ptr{Float64}, sg::Ptr{Float64})::Int32)
    one = y isa AbstractVector
    sh(A) = one ? A[:, 1] : A
    S, Cc = _cplx(Sv), _cplx(Cv)
    (freq = (0:Nf-1) .* df, dirty = sh(_cplx(Dv)), window = _cplx(Wnv), residual = sh(_cplx(Rv)), components = sh(Cc), picks = sh(Int.(picks[1:nit, :]) .+ 1),
     pick_values = sh(_cplx(pvv)[1:nit, :]), spectrum = sh(S), power = sh(abs2.(S)), amplitude = sh(2 .* abs.(Cc)), iterations = one ? Int(iters[1]) : Int.(iters),
     status = one ? CLEAN_STATUS[status[1]+1] : [CLEAN_STATUS[v+1] for v in status], sigma = sg[1])
end
function clean_last_timing()
    tm = zeros(14)
    GC.@preserve tm check(@ccall LIB.lpvs_clean_last_timing(tm::Ptr{Float64}, Int32(14)::Int32)::Int32)
    (path = tm[1] == 1 ? :direct : tm[1] == 2 ? :nufft : :none, residual = tm[2] == 1 ? :lds : tm[2] == 2 ? :global : :none, threads = Int(tm[3]),
     lds_bytes = Int(tm[4]), iterations_min = Int(tm[5]), iterations_max = Int(tm[6]), admissible = Int(tm[7]), moments_ms = tm[8], sums_ms = tm[9],
     loop_ms = tm[10], restore_ms = tm[11], copy_ms = tm[12], total_ms = tm[13], sigma = tm[14])
end

# ---- the bootstrap of the Lomb-Scargle periodogram (extension; include/lpvspectral.h g6) -------------------------------------------------
"""    lombscargle_bootstrap(y, t, f=default_freqs(t); W=nothing, B=1000, seed=0, row0=0, fit_mean=true, center_data=true, normalization=:standard, power=false)
The maxima of the `lombscargle` periodograms of the resamples `row0 .. row0 + B - 1` of ONE record (`t` and `W` stay with the epochs), formed
on the device.  Returns `(maxima, argmax, means)` -- `argmax` 1-based -- and, with `power=true`, also the columns `Nf × B`."""
function lombscargle_bootstrap(y::AbstractVector{<:Real}, t::AbstractVector{<:Real}, f::AbstractVector{<:Real}=default_freqs(t); W=nothing, B::Integer=1000,
                               seed::Integer=0, row0::Integer=0, fit_mean::Bool=true, center_data::Bool=true, normalization::Symbol=:standard,
                               device::Integer=0, power::Bool=false)
    yv, tv, fv = Vector{Float64}(y), Vector{Float64}(t), Vector{Float64}(f)
    N, Nf = length(tv), length(fv)
    @assert length(yv) == N "y has to be as long as the sampling points"
    Wv = W === nothing ? Float64[] : Vector{Float64}(W)
    @assert W === nothing || length(Wv) == N "W has to be as long as the sampling points"
    Wp = W === nothing ? Ptr{Float64}(C_NULL) : pointer(Wv)
    nb = max(Int(B), 1)
    maxima, argmax, means = zeros(nb), zeros(Int64, nb), zeros(nb)
    pwv = power ? zeros(Nf, nb) : Float64[]
    pwp = power ? pointer(pwv) : Ptr{Float64}(C_NULL)
    GC.@preserve yv tv Wv fv maxima argmax means pwv check(@ccall LIB.lpvs_lombscargle_bootstrap_f64(yv::Ptr{Float64}, tv::Ptr{Float64}, Int64(N)::Int64,
        Wp::Ptr{Float64}, fv::Ptr{Float64}, Int64(Nf)::Int64, Int64(B)::Int64, Int64(seed)::Int64, Int64(row0)::Int64, Int32(fit_mean)::Int32,
        Int32(center_data)::Int32, LOMB_NORMALIZATIONS[normalization]::Int32, Int32(device)::Int32, maxima::Ptr{Float64}, argmax::Ptr{Int64},
        means::Ptr{Float64}, pwp::Ptr{Float64})::Int32)
    power ? (maxima, argmax .+ 1, means, pwv) : (maxima, argmax .+ 1, means)
end
function lombscargle_bootstrap_last_timing()
    tm = zeros(12)
    GC.@preserve tm check(@ccall LIB.lpvs_lombscargle_bootstrap_last_timing(tm::Ptr{Float64}, Int32(12)::Int32)::Int32)
    (resamples=Int(tm[1]), chunks=Int(tm[2]), ts=Int(tm[3]), slab=Int(tm[4]), slabs=Int(tm[5]), degenerate=Int(tm[6]), shared_ms=tm[7], moments_ms=tm[8],
     sums_ms=tm[9], epilogue_ms=tm[10], copy_ms=tm[11], total_ms=tm[12])
end

_quantile_pair(q::Number) = (q = q < 0.5 ? q : 1 - q; (Float64(q), Float64(1 - q)))                      # src/plotting.jl:39-44
_quantile_pair(q) = (Float64(min(q...)), Float64(max(q...)))

# clamp of x (take_log: of log.(x)) to its own quantiles; x is a column-major matrix or a view of one with unit row stride
function _compress(x::AbstractVecOrMat{<:Real}, q, take_log::Bool; device::Integer = 0)
    qlo, qhi = _quantile_pair(q)
    rows, cols = size(x, 1), size(x, 2)
    th = zeros(Float64, 2)
    if eltype(x) == Float32
        xv = Matrix{Float32}(reshape(x, rows, cols)); out32 = Matrix{Float32}(undef, rows, cols)
        GC.@preserve xv out32 th check(@ccall LIB.lpvs_compress_f32(xv::Ptr{Float32}, Int64(rows)::Int64, Int64(cols)::Int64, Int64(rows)::Int64,
            Int32(take_log)::Int32, qlo::Float64, qhi::Float64, Int32(device)::Int32, out32::Ptr{Float32}, Int64(rows)::Int64, th::Ptr{Float64})::Int32)
        return (x isa AbstractVector ? vec(out32) : out32), (th[1], th[2])
    end
    xw = Matrix{Float64}(reshape(x, rows, cols)); out64 = Matrix{Float64}(undef, rows, cols)
    GC.@preserve xw out64 th check(@ccall LIB.lpvs_compress_f64(xw::Ptr{Float64}, Int64(rows)::Int64, Int64(cols)::Int64, Int64(rows)::Int64,
        Int32(take_log)::Int32, qlo::Float64, qhi::Float64, Int32(device)::Int32, out64::Ptr{Float64}, Int64(rows)::Int64, th::Ptr{Float64})::Int32)
    (x isa AbstractVector ? vec(out64) : out64), (th[1], th[2])
end

compress(x, q; device::Integer = 0) = _compress(x, q, false; device=device)[1]                            # src/plotting.jl:38-47

# the numbers of plot_spectrogram and of the MelSpectrogram recipe: (time, frequencies[2:end], compress(log.(power)[2:end, :], compression))
heatmap(S::Spectrogram; compression = (0.005, 1), device::Integer = 0) =
    (S.time, S.freq[2:end], _compress(S.power[2:end, :], compression, true; device=device)[1])
_mel_to_hz(m) = m >= 1000f0 / (200f0 / 3) ? 1000f0 * exp((log(6.4f0) / 27f0) * (m - 1000f0 / (200f0 / 3))) : (200f0 / 3) * m   # src/mel.jl:56-71
heatmap(M::MelSpectrogram; compression = (0.005, 1), device::Integer = 0) =
    (M.time, _mel_to_hz.(M.mels)[2:end], _compress(M.power[2:end, :], compression, true; device=device)[1])

end # module
