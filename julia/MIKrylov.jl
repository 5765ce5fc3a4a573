# MIKrylov.jl -- Julia shim that makes libexpv_mi.so (the MI355X Krylov exp(tA)v engine) a drop-in for the Krylov
# path of SciML/ExponentialUtilities.jl: device-resident array / operator / KrylovSubspace types, and methods of the
# reference's own generic functions (arnoldi!, lanczos!, expv!, phiv!, _phiv!, phiv_timestep!, expv_timestep!, kiops,
# _phiv_timestep_caches, the error-estimate expv!) that forward to the C ABI of include/expv_mi.h with `ccall`.
# OrdinaryDiffEq's exponential integrators keep calling the reference API; dispatch on MIVector / MIOperator picks
# these methods.
#
# STATUS: source only.  The build image has no Julia, so this file has never been executed; what IS checked here:
#   * method signatures were checked by hand against the reference's for dispatch ambiguities (a method that is more specific in
#     one argument and less in another is a MethodError at the first call): expv! is split into `t::Real` / `t::Complex` like
#     krylov_phiv.jl:200-203, :252-255 for that reason,
#   * every `ccall` below names an exported symbol with the argument order of include/expv_mi.h
#     (tests/test_abi_cpu.py::test_julia_shim_calls_match_the_header),
#   * the option structs restated below have the library's field order and types
#     (tests/test_abi_cpu.py::test_struct_layouts_match_the_library; at load time `check_abi()` repeats that check
#     against expv_mi_abi_sizeof, so a mismatched library refuses to load),
#   * the identical entry points with the identical marshalling are exercised by the Python/ctypes mirror
#     (exponentialutilities.jl_amd/api.py) in the -m gpu parity tests.
#
# Reference methods replaced (all under /root/reference/src/):
#   arnoldi.jl:50-93,161-180,345-377,456-490   KrylovSubspace storage, arnoldi, arnoldi!, lanczos!
#   krylov_phiv.jl:125-168,200-280,563-653       expv, expv!, phiv, phiv!, _phiv!
#   krylov_phiv_adaptive.jl:57-114,184-232,260-453,502-511   expv_timestep(!), phiv_timestep(!), _phiv_timestep_caches
#   kiops.jl:57-281                               kiops
#   krylov_phiv_error_estimate.jl:96-101,149-207  get_subspace_cache, expv!(w,t,A,b,Ks,cache)
module MIKrylov

using LinearAlgebra, SparseArrays
import ExponentialUtilities
import ExponentialUtilities: KrylovSubspace, arnoldi, arnoldi!, lanczos!, expv, expv!, phiv, phiv!, _phiv!,
                             phiv_timestep, phiv_timestep!, expv_timestep, expv_timestep!, kiops,
                             _phiv_timestep_caches, get_subspace_cache, getV, getH

const lib = get(ENV, "EXPV_MI_LIB", joinpath(@__DIR__, "..", "exponentialutilities.jl_amd", "libexpv_mi.so"))
const F64, C64, F32, C32 = Cint(0), Cint(1), Cint(2), Cint(3)
const HOST, DEVICE = Cint(0), Cint(1)
# every BlasFloat (ExponentialUtilities.jl:19): the 32-bit types run natively on 32-bit storage (two-kernel step, fp64 projection
# sums); kiops is Float64-only like the reference method and answers Unsupported for them
const MIScalar = Union{Float64, ComplexF64, Float32, ComplexF32}
dtype(::Type{Float64}) = F64
dtype(::Type{ComplexF64}) = C64
dtype(::Type{Float32}) = F32
dtype(::Type{ComplexF32}) = C32

# ---- option / result structs: field order and types of include/expv_mi.h (verified by check_abi) ----------------
struct ArnoldiOpts
    m::Cint
    iop::Cint
    init::Cint
    ishermitian::Cint
    ortho::Cint
    flags::Cint
    tol::Cdouble
end
struct ExpvStats
    m_used::Cint
    wasbreakdown::Cint
    matvecs::Cint
    path_flags::Cint
    beta::Cdouble
end
struct TimestepOpts
    tau::Cdouble
    tol::Cdouble
    delta::Cdouble
    gamma::Cdouble
    opnorm::Cdouble
    has_opnorm::Cint
    m::Cint
    iop::Cint
    correct::Cint
    adaptive::Cint
    ishermitian::Cint
    verbose::Cint
    ortho::Cint
    no_basis_reuse::Cint
    reserved::Cint
    NA::Int64
    print::Ptr{Cvoid}
    print_user::Ptr{Cvoid}
end
struct TimestepStats
    num_timesteps::Cint
    matvecs::Cint
    m_final::Cint
    arnoldi_calls::Cint
    arnoldi_reused::Cint
    stalled_steps::Cint
end
struct KiopsOpts
    mmin::Cint
    mmax::Cint
    m::Cint
    iop::Cint
    ishermitian::Cint
    task1::Cint
    ortho::Cint
    reserved::Cint
    tol::Cdouble
end
function check_abi()
    for (kind, T) in ((0, ArnoldiOpts), (1, ExpvStats), (2, TimestepOpts), (3, TimestepStats), (4, KiopsOpts))
        want = ccall((:expv_mi_abi_sizeof, lib), Csize_t, (Cint,), kind)
        want == sizeof(T) || error("libexpv_mi.so: $(T) is $(want) bytes in the library, $(sizeof(T)) here")
    end
end

# ---- context: one GPU + one HIP stream --------------------------------------------------------------------------
mutable struct Ctx
    h::Ptr{Cvoid}
end
function Ctx(device::Integer = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_ctx_create, lib), Cint, (Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, r), C_NULL)
    c = Ctx(r[])
    # Julia runs finalizers in no particular order at exit: the library expects that -- expv_mi_ctx_destroy clears the back
    # pointers of the operator / KrylovSubspace / cache handles that outlive it, and their own destroy then only frees their
    # device memory (tests/test_gpu_configs.py: test_handles_may_outlive_their_context...; tests/c_harness does exactly this)
    finalizer(c -> (ccall((:expv_mi_ctx_destroy, lib), Cint, (Ptr{Cvoid},), c.h); c.h = C_NULL), c)
    c
end
const CTX = Ref{Ctx}()
ctx() = (isassigned(CTX) || (check_abi(); CTX[] = Ctx()); CTX[])
sync() = check(ccall((:expv_mi_ctx_sync, lib), Cint, (Ptr{Cvoid},), ctx().h), ctx().h)
# engine options of the context by name ("pipeline", "wave", "fused", "dia", "mailbox", "nontemporal", "stencil", ...: expv_mi.h)
set_option!(name::AbstractString, value::Integer) =
    check(ccall((:expv_mi_ctx_set_option, lib), Cint, (Ptr{Cvoid}, Cstring, Int64), ctx().h, name, value), ctx().h)
function get_option(name::AbstractString)
    v = Ref{Int64}(0)
    check(ccall((:expv_mi_ctx_get_option, lib), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), ctx().h, name, v), ctx().h)
    v[]
end
# cumulative counters: Krylov steps, factorisations, on the single-pass step, overlapped, redone serially, redone without the
# wave form, operator applications outside a factorisation, factorisations whose H came home by copy (not the mailbox)
function counters()
    out = zeros(Int64, 8)
    check(ccall((:expv_mi_ctx_counters, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), ctx().h, out), ctx().h)
    out
end

# device self-test of the kernels' cross-lane sums (mismatching lanes per class; all zero when healthy)
function selftest()
    out = zeros(Int64, 8)
    check(ccall((:expv_mi_ctx_selftest, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), ctx().h, out), ctx().h)
    out
end

function check(code::Integer, h)
    code == 0 && return nothing
    msg = unsafe_string(ccall((:expv_mi_last_error, lib), Cstring, (Ptr{Cvoid},), h))
    code == 1 && throw(DimensionMismatch(msg))
    # (where the reference's `ceil(Int, x)` meets a non-finite x -- kiops.jl:210, krylov_phiv_adaptive.jl:470 -- it throws InexactError)
    code == 2 && occursin("InexactError", msg) && throw(InexactError(:ceil, Int, NaN))
    code == 2 && throw(ArgumentError(msg))
    code == 3 && throw(AssertionError(msg))
    code == 4 && throw(LinearAlgebra.SingularException(0))
    code == 6 && throw(OutOfMemoryError())
    code == 8 && throw(BoundsError())
    error("expv_mi status $code: $msg")          # 5 (error(...) in the reference), 7 (HIP)
end

# ---- device arrays (column-major, like Array) ---------------------------------------------------------------------
mutable struct MIArray{T, N} <: AbstractArray{T, N}
    ptr::Ptr{Cvoid}
    dims::NTuple{N, Int}
    owned::Bool
end
const MIVector{T} = MIArray{T, 1}
const MIMatrix{T} = MIArray{T, 2}
const MIVecOrMat{T} = Union{MIVector{T}, MIMatrix{T}}
Base.size(a::MIArray) = a.dims
Base.IndexStyle(::Type{<:MIArray}) = IndexLinear()
Base.getindex(a::MIArray, i...) = error("MIArray lives in HBM: copy it to the host with Array(a) first")
Base.show(io::IO, a::MIArray{T}) where {T} = print(io, join(a.dims, "x"), " MIArray{", T, "} in HBM @", a.ptr)      # (the generic show would index)
Base.show(io::IO, ::MIME"text/plain", a::MIArray) = show(io, a)
function MIArray{T}(::UndefInitializer, dims::Vararg{Int, N}) where {T <: MIScalar, N}
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_malloc, lib), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), ctx().h, max(prod(dims), 1) * sizeof(T), r), ctx().h)
    a = MIArray{T, N}(r[], dims, true)
    # (never ctx() here: a finalizer must not create a context, and the context's own finalizer may have run already --
    #  expv_mi_free does not dereference the handle it is given)
    finalizer(a -> a.owned && ccall((:expv_mi_free, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), isassigned(CTX) ? CTX[].h : C_NULL, a.ptr), a)
    a
end
MIArray{T, N}(::UndefInitializer, dims::Vararg{Int, N}) where {T, N} = MIArray{T}(undef, dims...)      # VType(undef, rows, cols), arnoldi.jl:68
Base.similar(a::MIArray, ::Type{T}, dims::Dims) where {T} = MIArray{T}(undef, dims...)                # similar(b, T, (n, m+1)), arnoldi.jl:171
Base.similar(a::MIArray{T}, dims::Dims) where {T} = MIArray{T}(undef, dims...)
function MIArray(x::Array{T}) where {T <: MIScalar}
    d = MIArray{T}(undef, size(x)...)
    check(ccall((:expv_mi_memcpy_h2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{T}, Csize_t), ctx().h, d.ptr, x, sizeof(x)), ctx().h)
    d
end
function Base.Array(d::MIArray{T}) where {T}
    x = Array{T}(undef, d.dims)
    check(ccall((:expv_mi_memcpy_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{T}, Ptr{Cvoid}, Csize_t), ctx().h, x, d.ptr, sizeof(x)), ctx().h)
    x
end
colptr(a::MIMatrix{T}, j::Integer) where {T} = a.ptr + (j - 1) * a.dims[1] * sizeof(T)
ld(a::MIVector) = max(a.dims[1], 1)
ld(a::MIMatrix) = max(a.dims[1], 1)
ncols(a::MIVector) = 1
ncols(a::MIMatrix) = a.dims[2]

# ---- dense matrices in HBM: exponential!(A) for a GPU array (exp.jl:56-58), mul!(C, A, B, alpha, beta) -----------------
# Computed on the device at every n (matrix-core products + a pivoted blocked LU).  Like the reference's GPU dispatch it runs
# ExpMethodHigham2005 WITHOUT balancing; unlike the generated evaluation graph it does not cap the scaling at 2^-8.
function ExponentialUtilities.exponential!(A::MIMatrix{T}) where {T <: MIScalar}
    n = LinearAlgebra.checksquare(A)
    info = zeros(Int64, 8)      # Pade order, squarings, row exchanges of the LU, microseconds
    check(ccall((:expv_mi_expm, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Cint, Ptr{Int64}),
                ctx().h, dtype(T), n, A.ptr, ld(A), DEVICE, info), ctx().h)
    A
end
# (do_balancing is ignored, as exp.jl:56-58 ignores it for an AbstractGPUArray)
ExponentialUtilities.exponential!(A::MIMatrix{T}, ::ExponentialUtilities.ExpMethodHigham2005, cache = nothing) where {T <: MIScalar} =
    ExponentialUtilities.exponential!(A)
# exponential!(A, ExpMethodHigham2005Base()) (exp_baseexp.jl:112-161), which the reference defines for a StridedMatrix only: gebal
# job 'B' on the device, the norm taken AFTER balancing, unbalance folded into the copy into A.  The method for badly scaled A.
function ExponentialUtilities.exponential!(A::MIMatrix{T}, ::ExponentialUtilities.ExpMethodHigham2005Base, cache = nothing) where {T <: MIScalar}
    n = LinearAlgebra.checksquare(A)
    info = zeros(Int64, 8)      # Pade order, squarings, row exchanges, microseconds, ilo, ihi, sweeps, microseconds of balancing
    check(ccall((:expv_mi_expm_balanced, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Cint, Ptr{Int64}),
                ctx().h, dtype(T), n, A.ptr, ld(A), DEVICE, info), ctx().h)
    A
end
# LAPACK.gebal!('B', A) for a matrix in HBM: A balanced in place; returns (ilo, ihi, scale) with scale::Vector{Float64} on the host
function balance!(A::MIMatrix{T}) where {T <: MIScalar}
    n = LinearAlgebra.checksquare(A)
    ilo, ihi, scale = Ref{Int64}(1), Ref{Int64}(0), ones(Float64, n)
    check(ccall((:expv_mi_gebal, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Cint, Ref{Int64}, Ref{Int64}, Ptr{Cdouble}),
                ctx().h, dtype(T), n, A.ptr, ld(A), DEVICE, ilo, ihi, scale), ctx().h)
    Int(ilo[]), Int(ihi[]), scale
end
function LinearAlgebra.mul!(C::MIMatrix{T}, A::MIMatrix{T}, B::MIMatrix{T}, α::Number, β::Number) where {T <: MIScalar}
    m, n, k = size(C, 1), size(C, 2), size(A, 2)
    (size(A, 1) == m && size(B, 1) == k && size(B, 2) == n) || throw(DimensionMismatch("mul!: C is $(size(C)), A is $(size(A)), B is $(size(B))"))
    (T <: Real && !(isreal(α) && isreal(β))) && throw(InexactError(:mul!, T, α))
    check(ccall((:expv_mi_gemm, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Cdouble, Cdouble, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Cdouble, Cdouble, Ptr{Cvoid}, Int64),
                ctx().h, dtype(T), m, n, k, real(α), imag(α), A.ptr, ld(A), B.ptr, ld(B), real(β), imag(β), C.ptr, ld(C)), ctx().h)
    sync()
    C
end
LinearAlgebra.mul!(C::MIMatrix{T}, A::MIMatrix{T}, B::MIMatrix{T}) where {T <: MIScalar} = LinearAlgebra.mul!(C, A, B, true, false)

# phi!(out, A, k) (phi.jl:159-257): out[j + 1] <- phi_j(A), A unchanged.  Scaling and recovering with ONE Taylor core for all four
# element types (the reference: tabulated Pade for Float64 / ComplexF64, the basis-vector route for the others); `caches` and
# `expmethod` are accepted and ignored -- the workspace lives in the context.  A non-finite entry throws ArgumentError.
function ExponentialUtilities.phi!(out::Vector{<:MIMatrix{T}}, A::MIMatrix{T}, k::Integer; caches = nothing, expmethod = nothing) where {T <: MIScalar}
    n = LinearAlgebra.checksquare(A)
    0 <= k <= 16 || throw(ArgumentError("phi!: k must be in 0:16"))
    length(out) == k + 1 || throw(DimensionMismatch("phi!: out has $(length(out)) matrices, k + 1 = $(k + 1)"))
    all(o -> size(o) == (n, n), out) || throw(DimensionMismatch("phi!: every out[j] must be $(n)x$(n)"))
    ptrs = Ptr{Cvoid}[o.ptr for o in out]
    info = zeros(Int64, 8)      # Taylor degree, scalings, products, microseconds
    GC.@preserve out check(ccall((:expv_mi_phi, lib), Cint,
                                 (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Cvoid}, Int64, Ptr{Ptr{Cvoid}}, Int64, Cint, Ptr{Int64}),
                                 ctx().h, dtype(T), n, k, A.ptr, ld(A), ptrs, max(n, 1), DEVICE, info), ctx().h)
    out
end
ExponentialUtilities.phi(A::MIMatrix{T}, k::Integer; kwargs...) where {T <: MIScalar} =
    ExponentialUtilities.phi!([MIArray{T}(undef, size(A)...) for _ in 0:k], A, k; kwargs...)

# ---- operator: the contract of docs/src/interfaces.md:7-36 (eltype, size, mul!, ishermitian, opnorm) --------------
mutable struct MIOperator{T}
    h::Ptr{Cvoid}
    n::Int
    herm::Bool
    nnz::Int
    opnorm_inf::Float64
end
function wrap_operator(::Type{T}, h::Ptr{Cvoid}) where {T}
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), h, n, nz, hm, on, dt), ctx().h)
    op = MIOperator{T}(h, n[], hm[] != 0, nz[], on[])
    finalizer(o -> ccall((:expv_mi_op_destroy, lib), Cint, (Ptr{Cvoid},), o.h), op)
    op
end
function MIOperator(A::SparseMatrixCSC{T, Int64}) where {T <: MIScalar}          # Julia's own layout, 1-based
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_csc, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{T}, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), size(A, 1), A.colptr, A.rowval, A.nzval, 1, r), ctx().h)
    wrap_operator(T, r[])
end
# A refreshed in place on the same pattern (a Jacobian updated every step): refill the uploaded operator instead of building
# a new one -- the reference reads A at call time, this is how a caller tells the device copy.  ~10x cheaper than MIOperator(A).
function update_values!(op::MIOperator{T}, A::SparseMatrixCSC{T, Int64}) where {T <: MIScalar}
    length(A.nzval) == op.nnz && size(A, 1) == op.n || throw(DimensionMismatch("update_values!: same pattern as at creation required"))
    check(ccall((:expv_mi_op_update_values, lib), Cint, (Ptr{Cvoid}, Ptr{T}, Cint), op.h, A.nzval, HOST), ctx().h)
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), op.h, n, nz, hm, on, dt), ctx().h)
    op.herm = hm[] != 0
    op.opnorm_inf = on[]
    op
end
# How the library stores a sparse operator: reordered = true when it kept P A P' (P = reverse Cuthill-McKee, context option
# "reorder") because that puts an unstructured operator on the single-pass Krylov step.  Nothing changes for the caller: vectors
# go in and come out in A's own ordering, H / beta / results are those of arnoldi(A, b) (rounding apart).
function reorder_info(op::MIOperator)
    out = zeros(Int64, 4)
    check(ccall((:expv_mi_op_reorder_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), op.h, out), ctx().h)
    (reordered = out[1] != 0, bandwidth_before = out[2], bandwidth_after = out[3], setup_s = 1.0e-6 * out[4])
end
# ordering plans by pattern (process-wide): re-creating an operator with a pattern seen before reuses its row ordering / patch plan
function plan_cache(; clear::Bool = false, capacity::Union{Nothing, Integer} = nothing)
    out = zeros(Int64, 4)
    clear && check(ccall((:expv_mi_plan_cache, lib), Cint, (Cint, Int64, Ptr{Int64}), 1, 0, out), C_NULL)
    capacity === nothing || check(ccall((:expv_mi_plan_cache, lib), Cint, (Cint, Int64, Ptr{Int64}), 2, capacity, out), C_NULL)
    check(ccall((:expv_mi_plan_cache, lib), Cint, (Cint, Int64, Ptr{Int64}), 0, 0, out), C_NULL)
    (plans = out[1], hits = out[2], misses = out[3], capacity = out[4])
end
# 2-D grid stencils (context option "patch", default on): stored in a grid-patch ordering -- a special case of the reordering above,
# equally invisible to the caller.  patch_form, the row length of the recognised grid, tiles, longest / mean ring of a tile.
function patch_info(op::MIOperator)
    out = zeros(Int64, 8)
    check(ccall((:expv_mi_op_patch_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), op.h, out), ctx().h)
    (patch_form = out[1] != 0, grid_row_length = out[2], tiles = out[3], longest_ring = out[4], mean_ring = out[3] > 0 ? out[5] / out[3] : 0.0)
end
# Banded Float64 operators (context option "elide", default on): the (tile of 512 stored rows, diagonal) pairs on which the stored diagonal
# holds one value and is read as one entry instead of being streamed; mask[t] bit d-1 = diagonal d on tile t.
function elide_info(op::MIOperator)
    out = zeros(Int64, 4)
    check(ccall((:expv_mi_op_elide_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Int64), op.h, out, C_NULL, 0), ctx().h)
    mask = zeros(UInt8, out[1])
    isempty(mask) || check(ccall((:expv_mi_op_elide_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Int64), op.h, out, mask, length(mask)), ctx().h)
    (tiles = out[1], diagonals = out[2], constant_pairs = out[3], wholly_constant = out[4] != 0, mask = mask)
end
MIOperator(A::SparseMatrixCSC{T}) where {T <: MIScalar} = MIOperator(SparseMatrixCSC{T, Int64}(A))      # (other index types: converted once)
# A' and transpose(A) of an operator that exists (expv_mi_op_create_adjoint): the reference's expv(t, A', b), where A' is a lazy
# wrapper and mul! does the rest (arnoldi.jl:185) -- the call of an adjoint sensitivity and of a left eigenvector.  Here the
# result is a NEW, independent MIOperator built on the device from what A stores (sparse of any birth, or dense: an owned packed
# copy); the values never visit the host, and A may be updated or finalised afterwards.  Every A' builds a new operator: keep it.
# (A').opnorm_inf is opnorm(A, 1).  A matrix-free operator has no adjoint (Unsupported).
const OP_TRANSPOSE, OP_ADJOINT = Cint(1), Cint(2)
function adjoint_operator(A::MIOperator{T}, how::Cint) where {T}
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_adjoint, lib), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), A.h, how, r), ctx().h)
    wrap_operator(T, r[])
end
Base.adjoint(A::MIOperator) = adjoint_operator(A, OP_ADJOINT)
Base.transpose(A::MIOperator) = adjoint_operator(A, OP_TRANSPOSE)
# The refresh: dest -- made by adjoint(parent) or transpose(parent), and staying what it was made as -- takes the CURRENT values of
# parent (or of an operator of the same pattern) on the device; bit-equal to making it anew (expv_mi_op_adjoint_refresh).
function LinearAlgebra.adjoint!(dest::MIOperator{T}, parent::MIOperator{T}) where {T}
    check(ccall((:expv_mi_op_adjoint_refresh, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), dest.h, parent.h), ctx().h)
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), dest.h, n, nz, hm, on, dt), ctx().h)
    dest.herm = hm[] != 0
    dest.nnz = nz[]
    dest.opnorm_inf = on[]
    dest
end
# Linear combinations of operators that exist (expv_mi_op_create_lincomb): the reference's expv(t, H0 + f(tk)*H1, b) and
# expv(t, A - sigma*I, b), where + and * on a sparse matrix make the sum.  Here the result is a NEW, independent MIOperator built on
# the device from what the terms store (all sparse, of any birth, or all dense; one element type and size); the values never visit the
# host.  The pattern is the union of the terms' patterns (plus the diagonal with an identity term), whatever the values are --
# cancelled entries stay stored --, the values are added in term order, the identity last, nothing fused (include/expv_mi.h).
# lincomb(terms, coefs; identity) is the one-pass form for more than two terms (A + B + C builds A + B first); recombine! gives
# an operator made here new coefficients and the terms' current values for the cost of one kernel and a value refill.
const LINCOMB_IDENTITY = Cint(1)
const LINCOMB_KEPT = WeakKeyDict{Any, Any}()      # result => (terms, whether it holds the identity's diagonal)
function lincomb_pairs(coefs, identity)
    cs = identity === nothing ? collect(Number, coefs) : vcat(collect(Number, coefs), identity)
    pairs = Vector{Cdouble}(undef, 2 * length(cs))
    for (k, c) in enumerate(cs)
        pairs[2k - 1], pairs[2k] = real(c), imag(c)
    end
    pairs
end
function lincomb(terms::AbstractVector{MIOperator{T}}, coefs; identity = nothing) where {T}
    length(coefs) == length(terms) || throw(DimensionMismatch("lincomb: one coefficient per term expected"))
    isempty(terms) && throw(ArgumentError("lincomb: one term at least (the identity alone has no context, element type or size)"))
    hs, pairs = Ptr{Cvoid}[A.h for A in terms], lincomb_pairs(coefs, identity)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve terms check(ccall((:expv_mi_op_create_lincomb, lib), Cint, (Cint, Ptr{Ptr{Cvoid}}, Ptr{Cdouble}, Cint, Ref{Ptr{Cvoid}}),
                                   length(hs), hs, pairs, identity === nothing ? Cint(0) : LINCOMB_IDENTITY, r), ctx().h)
    C = wrap_operator(T, r[])
    LINCOMB_KEPT[C] = (collect(terms), identity !== nothing)
    C
end
function recombine!(C::MIOperator{T}, coefs, terms::Union{Nothing, AbstractVector{MIOperator{T}}} = nothing; identity = nothing) where {T}
    haskey(LINCOMB_KEPT, C) || throw(ArgumentError("recombine!: only an operator made by lincomb (or by + - * /) recombines"))
    kept, had = LINCOMB_KEPT[C]
    had == (identity !== nothing) || throw(ArgumentError("recombine!: give `identity` exactly when the operator was made with one"))
    terms === nothing && (terms = kept)      # the terms of the creation (or of the last recombine!)
    length(coefs) == length(terms) || throw(DimensionMismatch("recombine!: one coefficient per term expected"))
    hs, pairs = Ptr{Cvoid}[A.h for A in terms], lincomb_pairs(coefs, identity)
    GC.@preserve terms check(ccall((:expv_mi_op_lincomb_refresh, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cdouble}),
                                   C.h, length(hs), hs, pairs), ctx().h)
    LINCOMB_KEPT[C] = (collect(terms), identity !== nothing)
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), C.h, n, nz, hm, on, dt), ctx().h)
    C.herm = hm[] != 0
    C.nnz = nz[]
    C.opnorm_inf = on[]
    C
end
Base.:+(A::MIOperator{T}, B::MIOperator{T}) where {T} = lincomb([A, B], (1, 1))
Base.:-(A::MIOperator{T}, B::MIOperator{T}) where {T} = lincomb([A, B], (1, -1))
Base.:-(A::MIOperator) = lincomb([A], (-1,))
Base.:*(c::Number, A::MIOperator) = lincomb([A], (c,))
Base.:*(A::MIOperator, c::Number) = lincomb([A], (c,))
Base.:/(A::MIOperator, c::Number) = lincomb([A], (inv(c),))      # (the reciprocal is rounded first, then every entry multiplied)
Base.:+(A::MIOperator, J::UniformScaling) = lincomb([A], (1,); identity = J.λ)
Base.:-(A::MIOperator, J::UniformScaling) = lincomb([A], (1,); identity = -J.λ)
# A lazy A' / transpose(A) of a host SparseMatrixCSC needs no device transposition: the parent's CSC arrays ARE the CSR arrays of
# the transpose (columns sorted by row = rows sorted by column); the values are conjugated for an Adjoint.
function MIOperator(A::Union{Adjoint{T, SparseMatrixCSC{T, Int64}}, Transpose{T, SparseMatrixCSC{T, Int64}}}) where {T <: MIScalar}
    P = parent(A)
    vals = A isa Adjoint ? conj(P.nzval) : P.nzval
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_csr, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), size(P, 1), P.colptr, P.rowval, vals, 8, 1, r), ctx().h)
    wrap_operator(T, r[])
end
MIOperator(A::Adjoint{T, <:SparseMatrixCSC{T}}) where {T <: MIScalar} = MIOperator(adjoint(SparseMatrixCSC{T, Int64}(parent(A))))
MIOperator(A::Transpose{T, <:SparseMatrixCSC{T}}) where {T <: MIScalar} = MIOperator(transpose(SparseMatrixCSC{T, Int64}(parent(A))))
# A sparse matrix that is ALREADY on the device (test/gpu/gputests.jl:46: CuSparseMatrixCSR(A)): the three arrays of a CSR / CSC matrix
# as device vectors -- the fields of a ROCSparseMatrixCSR (rowPtr, colVal, nzVal) or ROCSparseMatrixCSC (colPtr, rowVal, nzVal), wrapped
# without a copy as MIArray{Ti, 1}(pointer, (length,), false); 1-based like every Julia sparse type.  The index arrays are checked on
# the device, only the pattern visits the host (the orderings and storage layouts are planned there), the values stay where they are.
# The arrays are read during the call only.  update_values!(op, nzval::MIVector) refreshes the values in the same entry order.
# format = :coo takes coordinate triplets instead: first vector = I, second = J, third = V (see the host method below).
function MIOperator(rowptr::MIVector{Ti}, colval::MIVector{Ti}, nzval::MIVector{T}, n::Integer;
                    format::Symbol = :csr, index_base::Integer = 1) where {Ti <: Union{Int32, Int64}, T <: MIScalar}
    format in (:csr, :csc, :coo) || throw(ArgumentError("MIOperator: format must be :csr, :csc or :coo"))
    if format == :coo      # rowptr = I, colval = J, nzval = V: the arrays of a ROCSparseMatrixCOO (rowInd, colInd, nzVal), or what an assembly left
        length(rowptr) == length(colval) == length(nzval) || throw(DimensionMismatch("MIOperator: I, J and V must have the same length"))
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:expv_mi_op_create_coo_loc, lib), Cint,
                    (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
                    ctx().h, dtype(T), n, length(nzval), rowptr.ptr, colval.ptr, nzval.ptr, sizeof(Ti), index_base, DEVICE, r), ctx().h)
        return wrap_operator(T, r[])
    end
    length(rowptr) == n + 1 || throw(DimensionMismatch("MIOperator: the pointer array must have n + 1 entries"))
    length(colval) == length(nzval) || throw(DimensionMismatch("MIOperator: index and value arrays must have the same length"))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    if format == :csr
        check(ccall((:expv_mi_op_create_csr_loc, lib), Cint,
                    (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
                    ctx().h, dtype(T), n, length(nzval), rowptr.ptr, colval.ptr, nzval.ptr, sizeof(Ti), index_base, DEVICE, r), ctx().h)
    else
        check(ccall((:expv_mi_op_create_csc_loc, lib), Cint,
                    (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
                    ctx().h, dtype(T), n, length(nzval), rowptr.ptr, colval.ptr, nzval.ptr, sizeof(Ti), index_base, DEVICE, r), ctx().h)
    end
    wrap_operator(T, r[])
end
# Block-compressed arrays with square blocks, already on the device: the fields of a ROCSparseMatrixBSR (rowPtr, colVal, nzVal,
# blockDim, dir) -- block_dim is the fifth argument, format = :bsr (pointer array over block rows) or :bsc (over block columns),
# block_order = :row (nzVal[r, c, k] row-major inside a block, dir = 'R') or :col (dir = 'C').  n is the scalar size.  The operator is
# the scalar matrix with EVERY element of every stored block stored (op.nnz = length(nzval)); the block arrays are checked and
# expanded on the device.  update_values!(op, nzval::MIVector) refreshes the values in the same block order and layout.
function MIOperator(ptr::MIVector{Ti}, idx::MIVector{Ti}, nzval::MIVector{T}, n::Integer, block_dim::Integer;
                    format::Symbol = :bsr, block_order::Symbol = :row, index_base::Integer = 1) where {Ti <: Union{Int32, Int64}, T <: MIScalar}
    format in (:bsr, :bsc) || throw(ArgumentError("MIOperator: with a block dimension format must be :bsr or :bsc"))
    block_order in (:row, :col) || throw(ArgumentError("MIOperator: block_order must be :row or :col"))
    block_dim >= 1 && n % block_dim == 0 || throw(DimensionMismatch("MIOperator: n must be a multiple of block_dim"))
    length(ptr) == div(n, block_dim) + 1 || throw(DimensionMismatch("MIOperator: the pointer array must have n / block_dim + 1 entries"))
    length(nzval) == length(idx) * block_dim^2 || throw(DimensionMismatch("MIOperator: block_dim^2 values per block index expected"))
    layout = (block_order == :col ? 1 : 0) | (format == :bsc ? 2 : 0)      # EXPV_MI_BSR_BLOCK_COL_MAJOR, EXPV_MI_BSR_COMPRESSED_COLS
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_bsr_loc, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), n, length(idx), block_dim, ptr.ptr, idx.ptr, nzval.ptr, sizeof(Ti), index_base, layout, DEVICE, r), ctx().h)
    wrap_operator(T, r[])
end
# Stored diagonals (DIA / banded storage, expv_mi_op_create_dia_loc): `data` holds one diagonal per COLUMN (Julia is column-major:
# column d is row d of the C interface, size(data, 1) its ld), `offsets[d]` its offset k = column - row, in any order.  align says
# where A[i, i + k] lies in its column: :col at (1-based) index i + k (the rows of a LAPACK band matrix, scipy's dia_matrix), :row
# at index i (the DIA of GPU sparse libraries), :start at index min(i, i + k) (compact vectors, what Tridiagonal holds).  The
# pattern is decided by the offsets alone -- every in-matrix position of a stored diagonal is a stored entry, zeros included, rows
# sorted whatever the order of `offsets` -- and slots that correspond to no matrix position are never read.  The data of an MIMatrix
# is expanded where it is; a host Matrix is staged and takes the same path.  update_values!(op, data) refreshes the values from an
# array of the same size and alignment.
const DIA_ALIGN = Dict(:col => 0, :row => 1, :start => 2)      # EXPV_MI_DIA_ALIGN_COL, _ROW, _START
function dia_create(::Type{T}, n::Integer, offsets::Vector{Int64}, data, ldv::Integer, align::Symbol, loc::Integer) where {T <: MIScalar}
    haskey(DIA_ALIGN, align) || throw(ArgumentError("MIOperator: align must be :col, :row or :start"))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve offsets data check(ccall((:expv_mi_op_create_dia_loc, lib), Cint,
                                         (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Int64}, Ptr{Cvoid}, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
                                         ctx().h, dtype(T), n, length(offsets), offsets, data, ldv, DIA_ALIGN[align], loc, r), ctx().h)
    wrap_operator(T, r[])
end
function MIOperator(data::MIMatrix{T}, offsets::AbstractVector{<:Integer}, n::Integer; format::Symbol = :dia, align::Symbol = :col) where {T <: MIScalar}
    format == :dia || throw(ArgumentError("MIOperator: a matrix of diagonals and their offsets take format = :dia"))
    size(data, 2) == length(offsets) || throw(DimensionMismatch("MIOperator: one column of data per offset expected"))
    dia_create(T, n, collect(Int64, offsets), data.ptr, ld(data), align, DEVICE)
end
function MIOperator(data::Matrix{T}, offsets::AbstractVector{<:Integer}, n::Integer; format::Symbol = :dia, align::Symbol = :col) where {T <: MIScalar}
    format == :dia || throw(ArgumentError("MIOperator: a matrix of diagonals and their offsets take format = :dia"))
    size(data, 2) == length(offsets) || throw(DimensionMismatch("MIOperator: one column of data per offset expected"))
    dia_create(T, n, collect(Int64, offsets), pointer(data), max(size(data, 1), 1), align, HOST)
end
# LinearAlgebra's structured matrices: their vectors packed into :start alignment (column d = the diagonal from its first entry on)
function dia_pack(::Type{T}, n::Integer, vecs) where {T}
    data = zeros(T, max(n, 1), length(vecs))
    for (d, v) in enumerate(vecs)
        copyto!(view(data, 1:length(v), d), v)
    end
    data
end
dia_parts(A::Tridiagonal) = (Int64[-1, 0, 1], (A.dl, A.d, A.du))
dia_parts(A::SymTridiagonal) = (m = size(A, 1) - 1; (Int64[-1, 0, 1], (view(A.ev, 1:m), A.dv, view(A.ev, 1:m))))      # (ev may have n entries)
dia_parts(A::Bidiagonal) = (Int64[0, A.uplo == 'U' ? 1 : -1], (A.dv, A.ev))
dia_parts(A::Diagonal) = (Int64[0], (A.diag,))
const DiaStructured{T} = Union{Tridiagonal{T}, SymTridiagonal{T}, Bidiagonal{T}, Diagonal{T}}
function MIOperator(A::DiaStructured{T}) where {T <: MIScalar}
    n = size(A, 1)
    offsets, vecs = dia_parts(A)
    MIOperator(dia_pack(T, n, vecs), offsets, n; align = :start)
end
function update_values!(op::MIOperator{T}, data::Union{MIMatrix{T}, Matrix{T}}) where {T <: MIScalar}      # a diagonal-born operator: the creation's layout
    loc = data isa MIMatrix ? DEVICE : HOST
    GC.@preserve data check(ccall((:expv_mi_op_update_values, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), op.h, data isa MIMatrix ? data.ptr : pointer(data), loc), ctx().h)
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), op.h, n, nz, hm, on, dt), ctx().h)
    op.herm = hm[] != 0
    op.opnorm_inf = on[]
    op
end
function update_values!(op::MIOperator{T}, A::DiaStructured{T}) where {T <: MIScalar}      # the same structured type as at creation
    size(A, 1) == op.n || throw(DimensionMismatch("update_values!: same size as at creation required"))
    update_values!(op, dia_pack(T, op.n, dia_parts(A)[2]))
end
# values a triplet-born operator takes at a refresh: one per triplet of the creation (repeats included); otherwise one per stored entry
nvalues(op::MIOperator) = (e = ingest_info(op).coo_entries; e > 0 ? e : op.nnz)
function update_values!(op::MIOperator{T}, nzval::MIVector{T}) where {T <: MIScalar}      # new values on the device, the creation's entry order
    length(nzval) == nvalues(op) || throw(DimensionMismatch("update_values!: one value per entry of the creation expected"))
    check(ccall((:expv_mi_op_update_values, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), op.h, nzval.ptr, DEVICE), ctx().h)
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), op.h, n, nz, hm, on, dt), ctx().h)
    op.herm = hm[] != 0
    op.opnorm_inf = on[]
    op
end
# sparse(I, J, V, n, n) without the detour: triplets in any order, entries of one coordinate ADDED -- in the element type, in
# ascending order of their position (the order is part of the library's contract: the same triplets give the same bits) --, a sum
# that comes out as zero stays stored.  The host arrays are staged into device memory and sorted / coalesced / compressed there,
# the path the device arrays of the constructor above take with format = :coo.  update_values!(op, V) then takes one value per
# triplet, in triplet order: a Jacobian re-assembled on a fixed mesh.
function MIOperator(I::Vector{Ti}, J::Vector{Ti}, V::Vector{T}, n::Integer; index_base::Integer = 1) where {Ti <: Union{Int32, Int64}, T <: MIScalar}
    length(I) == length(J) == length(V) || throw(DimensionMismatch("MIOperator: I, J and V must have the same length"))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_coo_loc, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Ti}, Ptr{Ti}, Ptr{T}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), n, length(V), I, J, V, sizeof(Ti), index_base, HOST, r), ctx().h)
    wrap_operator(T, r[])
end
function update_values!(op::MIOperator{T}, V::Vector{T}) where {T <: MIScalar}            # new values on the host, the creation's entry order
    length(V) == nvalues(op) || throw(DimensionMismatch("update_values!: one value per entry of the creation expected"))
    check(ccall((:expv_mi_op_update_values, lib), Cint, (Ptr{Cvoid}, Ptr{T}, Cint), op.h, V, HOST), ctx().h)
    n, nz, hm, on, dt = Ref{Int64}(0), Ref{Int64}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_op_info, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}), op.h, n, nz, hm, on, dt), ctx().h)
    op.herm = hm[] != 0
    op.opnorm_inf = on[]
    op
end
# what operator creation brought to the host (expv_mi_op_ingest_info): for an operator made from device arrays the pattern only
function ingest_info(op::MIOperator)
    out = zeros(Int64, 8)
    check(ccall((:expv_mi_op_ingest_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), op.h, out), ctx().h)
    (from_device = out[1] != 0, pattern_bytes_to_host = out[2], value_bytes_to_host = out[3], create_s = 1.0e-6 * out[4],
     ingest_s = 1.0e-6 * out[5], plan_cached = out[6] != 0, coo_entries = out[7], sort_passes = out[8])
end
function MIOperator(A::Matrix{T}) where {T <: MIScalar}
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_dense, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{T}, Int64, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), size(A, 1), A, max(size(A, 1), 1), HOST, r), ctx().h)
    wrap_operator(T, r[])
end
function MIOperator(A::MIMatrix{T}) where {T}                                    # already in HBM (the caller keeps it alive)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_dense, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), size(A, 1), A.ptr, ld(A), DEVICE, r), ctx().h)
    wrap_operator(T, r[])
end
# Matrix-free operator: anything that implements the reference's operator contract (docs/src/interfaces.md:7-36, exercised by
# test/basictests.jl:786-816): eltype, size, LinearAlgebra.mul!(y, A, x) on device vectors, ishermitian.  The library calls
# back with device pointers on its stream; the Julia object is kept alive by the operator that wraps it.
struct MatVecBox
    A::Any
    T::DataType
    n::Int
end
const MATVEC_ROOTS = IdDict{Ptr{Cvoid}, Any}()                # callback user pointer -> boxed operator (rooted while the handle lives)
function matvec_trampoline(user::Ptr{Cvoid}, xp::Ptr{Cvoid}, yp::Ptr{Cvoid}, stream::Ptr{Cvoid})::Cint
    try
        box = unsafe_pointer_to_objref(user)::Base.RefValue{MatVecBox}
        b = box[]
        x = MIArray{b.T, 1}(xp, (b.n,), false)
        y = MIArray{b.T, 1}(yp, (b.n,), false)
        LinearAlgebra.mul!(y, b.A, x)                          # the user's method, on MIVector arguments
        return Cint(0)
    catch
        return Cint(1)                                         # surfaces as ArgumentError from the library call
    end
end
function MIOperator(A, ::Type{T} = eltype(A); ishermitian::Bool = LinearAlgebra.ishermitian(A), nnz_hint::Integer = 0) where {T <: MIScalar}
    n = size(A, 1)
    box = Ref(MatVecBox(A, T, n))
    user = pointer_from_objref(box)
    fn = @cfunction(matvec_trampoline, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}))
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_op_create_callback, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), n, fn, user, ishermitian ? 1 : 0, nnz_hint, r), ctx().h)
    MATVEC_ROOTS[r[]] = box
    op = wrap_operator(T, r[])
    finalizer(o -> delete!(MATVEC_ROOTS, o.h), op)
    op
end
Base.eltype(::MIOperator{T}) where {T} = T
Base.size(A::MIOperator) = (A.n, A.n)
Base.size(A::MIOperator, d::Integer) = d <= 2 ? A.n : 1
LinearAlgebra.ishermitian(A::MIOperator) = A.herm
LinearAlgebra.opnorm(A::MIOperator, p::Real = Inf) = p == Inf ? A.opnorm_inf : error("MIOperator: only opnorm(A, Inf) is kept")
SparseArrays.nnz(A::MIOperator) = A.nnz
function LinearAlgebra.mul!(y::MIVector{T}, A::MIOperator{T}, x::MIVector{T}) where {T}                 # arnoldi.jl:185
    check(ccall((:expv_mi_op_apply, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint), A.h, x.ptr, DEVICE, y.ptr, DEVICE), ctx().h)
    y
end
# a REAL operator on complex vectors (expv_mi_op_apply_complex): the operator is read as it is stored, no promoted copy
const MIReal = Union{Float64, Float32}
function LinearAlgebra.mul!(y::MIVector{Complex{R}}, A::MIOperator{R}, x::MIVector{Complex{R}}) where {R <: MIReal}
    check(ccall((:expv_mi_op_apply_complex, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint), A.h, x.ptr, DEVICE, y.ptr, DEVICE), ctx().h)
    y
end

# ---- KrylovSubspace on the device ----------------------------------------------------------------------------------
# Ks.V is an MIMatrix over library-owned HBM; Ks.H stays a host Matrix{U} (arnoldi.jl:69) that WRAPS the library's host
# buffer (unsafe_wrap), so host code that edits H in place (kiops.jl:149-160, OrdinaryDiffEq reading Ks.H) keeps working.
mutable struct MIHandle
    h::Ptr{Cvoid}
    rows::Int            # n + augmented (Ks.V is padded: size(Ks.V, 1) is the leading dimension)
end
const HANDLES = WeakKeyDict{Any, MIHandle}()
handle(Ks) = HANDLES[Ks].h
function mi_subspace(::Type{T}, ::Type{U}, n::Integer, maxiter::Integer = 30, augmented::Integer = 0) where {T, U}
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_ks_create, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), dtype(U), n, maxiter, augmented, r), ctx().h)
    V, H = views_of(T, U, r[], n + augmented)
    Ks = KrylovSubspace{T, U, real(T), typeof(V), Matrix{U}}(maxiter, maxiter, augmented, zero(real(T)), false, V, H)
    hd = MIHandle(r[], n + augmented)
    finalizer(hd -> ccall((:expv_mi_ks_destroy, lib), Cint, (Ptr{Cvoid},), hd.h), hd)
    HANDLES[Ks] = hd
    Ks
end
function views_of(::Type{T}, ::Type{U}, h::Ptr{Cvoid}, rows::Integer) where {T, U}
    hp, ldh, nr, nc = Ref{Ptr{Cvoid}}(C_NULL), Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_ks_H, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Cint}, Ref{Cint}), h, hp, ldh, nr, nc), ctx().h)
    H = unsafe_wrap(Array, Ptr{U}(hp[]), (Int(ldh[]), Int(nc[])))
    vp, ldv = Ref{Ptr{Cvoid}}(C_NULL), Ref{Int64}(0)
    check(ccall((:expv_mi_ks_V_devptr, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}), h, vp, ldv), ctx().h)
    V = MIArray{T, 2}(vp[], (Int(ldv[]), size(H, 1)), false)       # library-owned: no finalizer; ldv >= rows (padded)
    V, H
end
# KrylovSubspace{T,U,MIMatrix{T}}(n, maxiter, augmented): the reference's own constructor form (arnoldi.jl:63-73)
KrylovSubspace{T, U, MIMatrix{T}}(n::Integer, maxiter::Integer = 30, augmented::Integer = false) where {T, U} =
    mi_subspace(T, U, n, maxiter, Int(augmented))
function sync_fields!(Ks)
    m, mi, aug, beta, wb = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0), Ref{Cdouble}(0), Ref{Cint}(0)
    check(ccall((:expv_mi_ks_get, lib), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ref{Cdouble}, Ref{Cint}),
                handle(Ks), m, mi, aug, beta, wb), ctx().h)
    Ks.m, Ks.beta, Ks.wasbreakdown = m[], beta[], wb[] != 0
    Ks
end
const MIKs{T, U} = KrylovSubspace{T, U, <:Any, <:MIMatrix}
function Base.resize!(Ks::MIKs{T, U}, maxiter::Integer) where {T, U}                                     # arnoldi.jl:80-93
    check(ccall((:expv_mi_ks_resize, lib), Cint, (Ptr{Cvoid}, Cint), handle(Ks), maxiter), ctx().h)
    Ks.V, Ks.H = views_of(T, U, handle(Ks), size(Ks.V, 1))        # the library reallocated both
    Ks.maxiter = maxiter
    sync_fields!(Ks)
end
# getV hands the caller an orthonormal basis: the library normalises lazily (expv_mi_ks_V_devptr materialises it)
function getV(Ks::MIKs{T, U}) where {T, U}
    vp, ldv = Ref{Ptr{Cvoid}}(C_NULL), Ref{Int64}(0)
    check(ccall((:expv_mi_ks_V_devptr, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}), handle(Ks), vp, ldv), ctx().h)
    MIArray{T, 2}(vp[], (Int(ldv[]), Ks.m + 1), false)       # leading dimension ldv >= rows; rows beyond n + augmented are zero padding
end

opts(m, tol, iop, init, herm; flags = 0) = Ref(ArnoldiOpts(m, iop, init, herm, 0, flags, tol))
const DEFER_TAIL = Cint(1)      # EXPV_MI_ARNOLDI_DEFER_TAIL: arnoldi! / lanczos! return before the closing pass has finished; every accessor below
                                # (getH, getV, Ks.m, expv!, phiv!, ...) goes through a library call that collects it

# arnoldi!(Ks, A, b; tol, m, ishermitian, opnorm, iop, init)                                  (src/arnoldi.jl:345-377)
function arnoldi!(Ks::MIKs{T, U}, A::MIOperator{T}, b::MIVector{T};
                  tol::Real = 1.0e-7, m::Int = min(Ks.maxiter, size(A, 1)), ishermitian::Bool = LinearAlgebra.ishermitian(A),
                  opnorm = nothing, iop::Int = 0, init::Int = 0, kw...) where {T, U}
    grow = m > Ks.maxiter
    check(ccall((:expv_mi_arnoldi, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{ArnoldiOpts}),
                handle(Ks), A.h, b.ptr, DEVICE, opts(m, tol, iop, init, ishermitian; flags = DEFER_TAIL)), ctx().h)
    grow && ((Ks.V, Ks.H) = views_of(T, U, handle(Ks), size(Ks.V, 1)); Ks.maxiter = m)         # resize!(Ks, m) happened inside (:355-357)
    sync_fields!(Ks)
end
# lanczos!(Ks, A, b; tol, m, ...)                                                              (src/arnoldi.jl:456-490)
function lanczos!(Ks::MIKs{T, U}, A::MIOperator{T}, b::MIVector{T};
                  tol::Real = 1.0e-7, m::Int = min(Ks.maxiter, size(A, 1)), opnorm = nothing, init::Int = 0, kw...) where {T, U}
    check(ccall((:expv_mi_lanczos, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{ArnoldiOpts}),
                handle(Ks), A.h, b.ptr, DEVICE, opts(m, tol, 0, init, 1; flags = DEFER_TAIL)), ctx().h)
    sync_fields!(Ks)
end
# arnoldi(A, b; m, ishermitian, kwargs...)                                                     (src/arnoldi.jl:161-180)
function arnoldi(A::MIOperator{T}, b::MIVector{T}; m = min(30, size(A, 1)),
                 ishermitian = LinearAlgebra.ishermitian(A), kw...) where {T}
    Ks = mi_subspace(T, ishermitian ? real(T) : T, length(b), m)
    arnoldi!(Ks, A, b; m = m, ishermitian = ishermitian, kw...)
end
# Mixed calls -- T = promote_type(eltype(A), eltype(b)) with a real A and a complex b (include/expv_mi.h: expv_mi_arnoldi): the same
# entries with the subspace and b of the operator's complex type; a real symmetric A runs lanczos! with U = R.  New dispatch only.
function arnoldi!(Ks::MIKs{Complex{R}, U}, A::MIOperator{R}, b::MIVector{Complex{R}};
                  tol::Real = 1.0e-7, m::Int = min(Ks.maxiter, size(A, 1)), ishermitian::Bool = LinearAlgebra.ishermitian(A),
                  opnorm = nothing, iop::Int = 0, init::Int = 0, kw...) where {R <: MIReal, U}
    grow = m > Ks.maxiter
    check(ccall((:expv_mi_arnoldi, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{ArnoldiOpts}),
                handle(Ks), A.h, b.ptr, DEVICE, opts(m, tol, iop, init, ishermitian; flags = DEFER_TAIL)), ctx().h)
    grow && ((Ks.V, Ks.H) = views_of(Complex{R}, U, handle(Ks), size(Ks.V, 1)); Ks.maxiter = m)
    sync_fields!(Ks)
end
function lanczos!(Ks::MIKs{Complex{R}, U}, A::MIOperator{R}, b::MIVector{Complex{R}};
                  tol::Real = 1.0e-7, m::Int = min(Ks.maxiter, size(A, 1)), opnorm = nothing, init::Int = 0, kw...) where {R <: MIReal, U}
    check(ccall((:expv_mi_lanczos, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{ArnoldiOpts}),
                handle(Ks), A.h, b.ptr, DEVICE, opts(m, tol, 0, init, 1; flags = DEFER_TAIL)), ctx().h)
    sync_fields!(Ks)
end
function arnoldi(A::MIOperator{R}, b::MIVector{Complex{R}}; m = min(30, size(A, 1)),
                 ishermitian = LinearAlgebra.ishermitian(A), kw...) where {R <: MIReal}
    Ks = mi_subspace(Complex{R}, ishermitian ? R : Complex{R}, length(b), m)
    arnoldi!(Ks, A, b; m = m, ishermitian = ishermitian, kw...)
end

# expv!(w, t, Ks; cache, expmethod)                                                           (src/krylov_phiv.jl:200-280)
# (the m x m exponential runs on the host inside the library: north_star; `cache` / `expmethod` are accepted and unused)
# Two methods with the reference's own split of `t` (krylov_phiv.jl:200-203 `t::Real`, :252-255 `t::Complex` with a complex w): one
# method on `t::Number` would be MORE specific than the reference's in w and Ks and LESS specific in t -- ambiguous for every call.
function _expv_ks!(w::MIVector{Tw}, t::Number, Ks) where {Tw}
    check(ccall((:expv_mi_expv_ks, lib), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Cint),
                handle(Ks), real(t), imag(t), w.ptr, DEVICE, dtype(Tw)), ctx().h)
    w
end
expv!(w::MIVector{Tw}, t::Real, Ks::MIKs{T, U}; cache = nothing, expmethod = nothing) where {Tw, T, U} = _expv_ks!(w, t, Ks)
expv!(w::MIVector{Complex{Tw}}, t::Complex{Tt}, Ks::MIKs{T, U}; cache = nothing, expmethod = nothing) where {Tw, Tt, T, U} =
    _expv_ks!(w, t, Ks)
# expv(t, A, b; kwargs...) in ONE library call (workspace reuse, no v_{m+1})                   (src/krylov_phiv.jl:135-144)
function ExponentialUtilities._expv_hb(t::Tt, A::MIOperator{T}, b::MIVector{T}; expmethod = nothing, cache = nothing,
                                       m = min(30, size(A, 1)), tol = 1.0e-7, iop = 0,
                                       ishermitian = LinearAlgebra.ishermitian(A), opnorm = nothing) where {Tt, T}
    w = similar(b, promote_type(Tt, T), (length(b),))
    st = Ref(ExpvStats(0, 0, 0, 0, 0.0))
    check(ccall((:expv_mi_expv, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Ref{ArnoldiOpts}, Ref{ExpvStats}),
                ctx().h, A.h, real(t), imag(t), b.ptr, DEVICE, w.ptr, DEVICE, dtype(eltype(w)), opts(m, tol, iop, 0, ishermitian), st), ctx().h)
    w
end
# expv(t, A, b) for a real A and a complex b (expv_mi_expv_realop): exp(-im * t * H) * psi with the real H as it is stored
function ExponentialUtilities._expv_hb(t::Tt, A::MIOperator{R}, b::MIVector{Complex{R}}; expmethod = nothing, cache = nothing,
                                       m = min(30, size(A, 1)), tol = 1.0e-7, iop = 0,
                                       ishermitian = LinearAlgebra.ishermitian(A), opnorm = nothing) where {Tt, R <: MIReal}
    w = similar(b, Complex{R}, (length(b),))
    st = Ref(ExpvStats(0, 0, 0, 0, 0.0))
    check(ccall((:expv_mi_expv_realop, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ref{ArnoldiOpts}, Ref{ExpvStats}),
                ctx().h, A.h, real(t), imag(t), b.ptr, DEVICE, w.ptr, DEVICE, opts(m, tol, iop, 0, ishermitian), st), ctx().h)
    w
end
# expv(t, A, b; mode = :error_estimate, ...)                                                  (src/krylov_phiv.jl:145-160)
# The reference's _expv_ee builds a HOST KrylovSubspace{T, U}(n, m), which cannot hold device vectors: the subspace is created on
# the device instead.  T = promote_type(typeof(t), eltype(A), eltype(b)) as there: a complex t (the Schroedinger case, -im) on a
# real operator needs the operator and b in the complex type -- MIOperator(ComplexF64.(A)) -- which the reference's generic mul!
# does implicitly.
function ExponentialUtilities._expv_ee(t::Tt, A::MIOperator{T}, b::MIVector{T}; m = min(30, size(A, 1)), tol = 1.0e-7, rtol = √(tol),
                                       ishermitian::Bool = LinearAlgebra.ishermitian(A), expmethod = nothing) where {Tt, T}
    Tp = promote_type(Tt, T)
    Tp == T || throw(ArgumentError("expv(...; mode = :error_estimate) with a $(Tt) time works in $(Tp): build the operator and b " *
                                   "in that type (MIOperator($(Tp).(A)), MIArray($(Tp).(b)))"))
    Ks = mi_subspace(T, ishermitian ? real(T) : T, length(b), m)
    w = similar(b, T, (length(b),))
    expv!(w, t, A, b, Ks, get_subspace_cache(Ks); atol = tol, rtol = rtol, ishermitian = ishermitian)
end
# phiv!(w, t, Ks, k; cache, correct, errest, expmethod) / _phiv!                              (src/krylov_phiv.jl:607-653)
function _phiv!(w::MIMatrix{Tw}, t::Number, Ks::MIKs{T, U}, k::Integer, cache, correct, expmethod) where {Tw, T, U}
    err = Ref{Cdouble}(0)
    check(ccall((:expv_mi_phiv_ks, lib), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cint, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Ref{Cdouble}),
                handle(Ks), real(t), imag(t), k, correct, w.ptr, ld(w), DEVICE, dtype(Tw), err), ctx().h)
    w, err[]
end
function phiv!(w::MIMatrix, t::Number, Ks::MIKs, k::Integer; cache = nothing, correct = false, errest = false, expmethod = nothing)
    w, err = _phiv!(w, t, Ks, k, cache, correct, expmethod)
    errest ? (w, err) : w
end
function phiv(t, A::MIOperator{T}, b::MIVector{T}, k; cache = nothing, correct = false, errest = false, kwargs_arnoldi...) where {T}
    Ks = arnoldi(A, b; kwargs_arnoldi...)
    w = MIArray{promote_type(typeof(t), T)}(undef, length(b), k + 1)
    phiv!(w, t, Ks, k; cache = cache, correct = correct, errest = errest)
end
function phiv(t, Ks::MIKs{T, U}, k; kwargs...) where {T, U}
    w = MIArray{promote_type(typeof(t), T)}(undef, HANDLES[Ks].rows, k + 1)
    phiv!(w, t, Ks, k; kwargs...)
end
function expv(t::Tt, Ks::MIKs{T, U}; expmethod = nothing, kwargs...) where {Tt, T, U}                  # krylov_phiv.jl:161-168
    w = MIArray{promote_type(Tt, T)}(undef, HANDLES[Ks].rows)
    expv!(w, t, Ks; kwargs...)
end

# ---- exp(tA)b without a Krylov basis: truncated Taylor series               (ext/ExponentialUtilitiesStaticArraysExt.jl:124-163) ----
# The reference has this algorithm for SMatrix, N <= 50, only (it lacks a norm estimator); names of their own, so that nothing here
# meets the reference's expv methods.  precision: 0 = working precision of real(T), 1 = the 2^-24 table in double arithmetic;
# opnorm: a bound on opnorm(A, Inf), matrix-free operators only.  A complex t needs a complex operator.
function expv_taylor!(w::MIVector{T}, t::Number, A::MIOperator{T}, b::MIVector{T}; precision::Integer = 0, max_matvecs::Integer = 0,
                      opnorm = nothing) where {T}
    length(w) == length(b) == size(A, 1) || throw(DimensionMismatch("length(w), length(b) and size(A, 1) must agree"))
    check(ccall((:expv_mi_expv_taylor, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}),
                ctx().h, A.h, real(t), imag(t), b.ptr, DEVICE, w.ptr, DEVICE, precision, max_matvecs,
                opnorm === nothing ? 0.0 : Float64(opnorm), C_NULL, C_NULL), ctx().h)
    w
end
expv_taylor(t::Number, A::MIOperator{T}, b::MIVector{T}; kw...) where {T} = expv_taylor!(similar(b, T, (length(b),)), t, A, b; kw...)
# A REAL operator with a complex time and complex vectors -- exp(-i t H) b with a real sparse H: the operator is read as it is stored
# (no promoted complex copy), w is complex, b is complex or real (widened on the device); w may be b only when b is complex.  On an
# operator with a fused form the values are those of expv_taylor on the promoted operator, element for element.
function expv_taylor!(w::MIVector{Complex{R}}, t::Number, A::MIOperator{R}, b::MIVector{Tb}; precision::Integer = 0, max_matvecs::Integer = 0,
                      opnorm = nothing) where {R <: Real, Tb <: Union{R, Complex{R}}}
    length(w) == length(b) == size(A, 1) || throw(DimensionMismatch("length(w), length(b) and size(A, 1) must agree"))
    check(ccall((:expv_mi_expv_taylor_realop, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Cint, Cint, Int64, Cdouble, Ptr{Int64}, Ptr{Cdouble}),
                ctx().h, A.h, real(t), imag(t), b.ptr, DEVICE, dtype(Tb), w.ptr, DEVICE, precision, max_matvecs,
                opnorm === nothing ? 0.0 : Float64(opnorm), C_NULL, C_NULL), ctx().h)
    w
end
expv_taylor(t::Number, A::MIOperator{R}, b::MIVector{Complex{R}}; kw...) where {R <: Real} = expv_taylor!(similar(b, Complex{R}, (length(b),)), t, A, b; kw...)
expv_taylor(t::Complex, A::MIOperator{R}, b::MIVector{R}; kw...) where {R <: Real} = expv_taylor!(similar(b, Complex{R}, (length(b),)), t, A, b; kw...)
# The same with the reference's WHOLE parameter search (:99-121): above the cheap threshold d_p = |t| ||(A - mu I)^p||^(1/p), p = 2 .. 9,
# are estimated on the device (opnorm_power) -- far fewer applications for a non-normal A; below it the call is expv_taylor!, bit
# for bit.  adjoint: an operator of A' (nothing: a Hermitian A serves as its own, otherwise one is made for the call).
function expv_taylor_power!(w::MIVector{T}, t::Number, A::MIOperator{T}, b::MIVector{T}; adjoint = nothing, precision::Integer = 0,
                            max_matvecs::Integer = 0) where {T}
    length(w) == length(b) == size(A, 1) || throw(DimensionMismatch("length(w), length(b) and size(A, 1) must agree"))
    check(ccall((:expv_mi_expv_taylor_power, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int64, Ptr{Int64}, Ptr{Cdouble}),
                ctx().h, A.h, adjoint === nothing ? C_NULL : adjoint.h, real(t), imag(t), b.ptr, DEVICE, w.ptr, DEVICE, precision, max_matvecs,
                C_NULL, C_NULL), ctx().h)
    w
end
expv_taylor_power(t::Number, A::MIOperator{T}, b::MIVector{T}; kw...) where {T} = expv_taylor_power!(similar(b, T, (length(b),)), t, A, b; kw...)
# A lower bound of opnorm((A - shift I)^p, q), q = Inf or 1, 1 <= p <= 16, by the deterministic block 1-norm estimator on the device
# (Higham & Tisseur 2000, t = 2); p = 1 with q = Inf is the exact row-sum norm.
function opnorm_power(A::MIOperator{T}, p::Integer, q::Real = Inf; shift::Number = 0.0, adjoint = nothing) where {T}
    q == Inf || q == 1 || throw(ArgumentError("opnorm_power: q must be Inf or 1"))
    est = Ref{Cdouble}(0.0)
    check(ccall((:expv_mi_op_norm_power, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cint, Ptr{Int64}, Ptr{Cdouble}),
                A.h, adjoint === nothing ? C_NULL : adjoint.h, p, Float64(real(shift)), Float64(imag(shift)), q == 1 ? 1 : 0, C_NULL, est), ctx().h)
    est[]
end
# A block of columns: size(B, 2) independent problems that share every pass over the operator; W[:, k] is bit for bit
# expv_taylor(t, A, B[:, k]).  W may be B.  A column that has stopped is masked but streamed until its panel of 8 has stopped.
function expv_taylor!(W::MIMatrix{T}, t::Number, A::MIOperator{T}, B::MIMatrix{T}; precision::Integer = 0, max_matvecs::Integer = 0,
                      opnorm = nothing) where {T}
    size(W) == size(B) && size(B, 1) == size(A, 1) || throw(DimensionMismatch("size(W), size(B) and size(A, 1) must agree"))
    check(ccall((:expv_mi_expv_taylor_block, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Cint, Int64,
                 Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}, Ptr{Cdouble}),
                ctx().h, A.h, real(t), imag(t), B.ptr, ld(B), ncols(B), 0, DEVICE, W.ptr, ld(W), 0, DEVICE, precision, max_matvecs,
                opnorm === nothing ? 0.0 : Float64(opnorm), C_NULL, C_NULL, C_NULL, C_NULL), ctx().h)
    W
end
expv_taylor(t::Number, A::MIOperator{T}, B::MIMatrix{T}; kw...) where {T} = expv_taylor!(similar(B, T, size(B)), t, A, B; kw...)
# A time grid: W[:, k] = exp(ts[k] t A) b in ONE sweep of the series -- the call is expv_taylor's for R t, R = max |ts|, and every other
# output is read off the terms of the stage it falls into, at no extra pass over the operator.  ts: real, all >= 0 or all <= 0 (the
# sign goes into t), any order, duplicates allowed; columns with |ts[k]| = R are bit for bit expv_taylor(R t, A, b); W may not overlap b.
function expv_taylor!(W::MIMatrix{T}, ts::AbstractVector{<:Real}, A::MIOperator{T}, b::MIVector{T}; t::Number = 1.0, precision::Integer = 0,
                      max_matvecs::Integer = 0, opnorm = nothing) where {T}
    size(W) == (length(b), length(ts)) && length(b) == size(A, 1) || throw(DimensionMismatch("size(W) must be (length(b), length(ts)) and length(b) == size(A, 1)"))
    any(>(0), ts) && any(<(0), ts) && throw(ArgumentError("expv_taylor: ts must be all >= 0 or all <= 0 (the sign is folded into t)"))
    r = Float64[abs(x) for x in ts]
    any(<(0), ts) && (t = -t)
    check(ccall((:expv_mi_expv_taylor_grid, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Cint, Int64,
                 Cdouble, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int64}),
                ctx().h, A.h, real(t), imag(t), r, length(r), b.ptr, DEVICE, W.ptr, ld(W), 0, DEVICE, precision, max_matvecs,
                opnorm === nothing ? 0.0 : Float64(opnorm), C_NULL, C_NULL, C_NULL), ctx().h)
    W
end
expv_taylor(ts::AbstractVector{<:Real}, A::MIOperator{T}, b::MIVector{T}; kw...) where {T} =
    expv_taylor!(similar(b, T, (length(b), length(ts))), ts, A, b; kw...)
# The result of phiv_timestep(t, A, B), B = [u_0 ... u_p] with p <= 8, by the same series on Al-Mohy & Higham's augmented matrix:
# w = sum_k t^k phi_k(tA) B[:, k].  No Krylov basis, no host exponential, three work vectors of length n; w may be B[:, 1].
function phiv_taylor!(w::MIVector{T}, t::Number, A::MIOperator{T}, B::MIMatrix{T}; precision::Integer = 0, max_matvecs::Integer = 0,
                      opnorm = nothing) where {T}
    length(w) == size(B, 1) == size(A, 1) || throw(DimensionMismatch("length(w), size(B, 1) and size(A, 1) must agree"))
    check(ccall((:expv_mi_phiv_taylor, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Cint, Cint, Int64, Cdouble,
                 Ptr{Int64}, Ptr{Cdouble}),
                ctx().h, A.h, real(t), imag(t), B.ptr, ld(B), ncols(B), 0, DEVICE, w.ptr, DEVICE, precision, max_matvecs,
                opnorm === nothing ? 0.0 : Float64(opnorm), C_NULL, C_NULL), ctx().h)
    w
end
phiv_taylor(t::Number, A::MIOperator{T}, B::MIMatrix{T}; kw...) where {T} = phiv_taylor!(similar(B, T, (size(B, 1),)), t, A, B; kw...)

# ---- error-estimate mode (Hermitian only)                                          (src/krylov_phiv_error_estimate.jl) ----
struct MISubspaceCache end                                                     # stands in for StegrCache: the library owns the scratch
get_subspace_cache(Ks::MIKs{T, U}) where {T, U <: Real} = MISubspaceCache()
get_subspace_cache(Ks::MIKs{T, U}) where {T, U <: Complex} =
    error("Subspace exponential caches not yet available for non-Hermitian matrices.")                 # :97
function expv!(w::MIVector{T}, t::Number, A::MIOperator{T}, b::MIVector{T}, Ks::MIKs{T, B}, cache::MISubspaceCache;
               atol::Real = 1.0e-8, rtol::Real = 1.0e-4, m = min(Ks.maxiter, size(A, 1)),
               ishermitian::Bool = LinearAlgebra.ishermitian(A), verbose::Bool = false, expmethod = nothing) where {T, B}
    check(ccall((:expv_mi_expv_error_estimate, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cdouble, Cdouble, Cint, Cint),
                handle(Ks), A.h, real(t), imag(t), b.ptr, DEVICE, w.ptr, DEVICE, atol, rtol, m, ishermitian), ctx().h)
    sync_fields!(Ks)
    w
end

# ---- time stepping                                                                    (src/krylov_phiv_adaptive.jl) ----
# _phiv_timestep_caches(u_prototype, maxiter, p)  (:502-511): the tuple shape (u, W, P, Ks, phiv_cache) is an
# implementation detail of the reference; here ONE opaque handle plays that role.
mutable struct MITimestepCaches
    h::Ptr{Cvoid}
    ts1::Vector{Float64}                                                          # _singleton_ts slot (:237-242)
end
function _phiv_timestep_caches(u_prototype::MIVector{T}, maxiter::Int, p::Int) where {T}
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:expv_mi_timestep_caches_create, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
                ctx().h, dtype(T), length(u_prototype), maxiter, p, r), ctx().h)
    c = MITimestepCaches(r[], [0.0])
    finalizer(c -> ccall((:expv_mi_timestep_caches_destroy, lib), Cint, (Ptr{Cvoid},), c.h), c)
    c
end
const PRINTLN = Ref{Ptr{Cvoid}}(C_NULL)
_println_cb(line::Cstring, ::Ptr{Cvoid}) = (println(unsafe_string(line)); nothing)
println_ptr() = (PRINTLN[] == C_NULL && (PRINTLN[] = @cfunction(_println_cb, Cvoid, (Cstring, Ptr{Cvoid}))); PRINTLN[])
# the library's slow-progress notice (>= 10^4 accepted sub-steps without step growth: the reference's controller keeps a tiny seed
# step, krylov_phiv_adaptive.jl:391-417) reaches the user as a warning even without `verbose`
const WARNLN = Ref{Ptr{Cvoid}}(C_NULL)
_warn_cb(line::Cstring, ::Ptr{Cvoid}) = (@warn unsafe_string(line); nothing)
warn_ptr() = (WARNLN[] == C_NULL && (WARNLN[] = @cfunction(_warn_cb, Cvoid, (Cstring, Ptr{Cvoid}))); WARNLN[])

# phiv_timestep!(U, ts, A, B; ...)  -- the whole controller runs in the library                 (:260-453)
function phiv_timestep!(U::MIVecOrMat{T}, ts::AbstractVector{tType}, A::MIOperator{T}, B::MIVecOrMat{T};
                        tau::Real = 0.0, m::Int = min(10, size(A, 1)), tol::Real = 1.0e-7, opnorm = nothing, iop::Int = 0,
                        correct::Bool = false, caches = nothing, adaptive = false, delta::Real = 1.2,
                        ishermitian::Bool = LinearAlgebra.ishermitian(A), gamma::Real = 0.8, NA::Int = 0,
                        verbose = false) where {T, tType <: Real}
    length(ts) == ncols(U) || throw(AssertionError("Dimension mismatch"))                              # :307
    (size(U, 1) == size(A, 1) == size(B, 1)) || throw(AssertionError("Dimension mismatch"))            # :308
    tsv = ts isa Vector{Float64} ? ts : Vector{Float64}(ts)                     # sorted IN PLACE by the library, like sort!(ts) (:297)
    has_opn, opn = 0, 0.0
    if opnorm !== nothing
        has_opn, opn = 1, Float64(opnorm isa Number ? opnorm : opnorm(A, Inf))  # a number or a function (:276-281)
    end
    o = Ref(TimestepOpts(tau, tol, delta, gamma, opn, has_opn, m, iop, correct, adaptive, ishermitian, verbose, 0, 0, 0, NA,
                         verbose ? println_ptr() : warn_ptr(), C_NULL))
    st = Ref(TimestepStats(0, 0, 0, 0, 0, 0))
    check(ccall((:expv_mi_phiv_timestep, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Int64, Cint,
                 Ref{TimestepOpts}, Ptr{Cvoid}, Ref{TimestepStats}),
                ctx().h, A.h, length(tsv), tsv, B.ptr, ld(B), ncols(B), DEVICE, U.ptr, ld(U), DEVICE, o,
                caches === nothing ? C_NULL : caches.h, st), ctx().h)
    tsv === ts || copyto!(ts, tsv)
    U
end
# scalar-time forms (:184-232, :99-114) and the allocating front ends (:57-67)
_singleton_ts(caches::MITimestepCaches, t::Float64) = (caches.ts1[1] = t; caches.ts1)
_singleton_ts(_, t) = [Float64(t)]
function phiv_timestep!(u::MIVector{T}, t::Real, A::MIOperator{T}, B::MIMatrix{T}; caches = nothing, kwargs...) where {T}
    phiv_timestep!(u, _singleton_ts(caches, t), A, B; caches = caches, kwargs...)
    u
end
function expv_timestep!(u::MIVector{T}, t::Real, A::MIOperator{T}, b::MIVector{T}; caches = nothing, kwargs...) where {T}
    phiv_timestep!(u, _singleton_ts(caches, t), A, b; caches = caches, kwargs...)
    u
end
expv_timestep!(U::MIMatrix{T}, ts::AbstractVector{<:Real}, A::MIOperator{T}, b::MIVector{T}; kwargs...) where {T} =
    phiv_timestep!(U, ts, A, b; kwargs...)
phiv_timestep(ts::Vector{<:Real}, A::MIOperator{T}, B::MIVecOrMat{T}; kwargs...) where {T} =
    phiv_timestep!(MIArray{T}(undef, size(A, 1), length(ts)), ts, A, B; kwargs...)
phiv_timestep(t::Real, A::MIOperator{T}, B::MIVecOrMat{T}; kwargs...) where {T} =
    phiv_timestep!(MIArray{T}(undef, size(A, 1)), [Float64(t)], A, B; kwargs...)
expv_timestep(ts::Vector{<:Real}, A::MIOperator{T}, b::MIVector{T}; kwargs...) where {T} = phiv_timestep(ts, A, b; kwargs...)
expv_timestep(t::Real, A::MIOperator{T}, b::MIVector{T}; kwargs...) where {T} = phiv_timestep(t, A, b; kwargs...)
# phiv_timestep! / expv_timestep! for a real A with complex B, U and caches (expv_mi_phiv_timestep_realop)
function phiv_timestep!(U::MIVecOrMat{Complex{R}}, ts::AbstractVector{tType}, A::MIOperator{R}, B::MIVecOrMat{Complex{R}};
                        tau::Real = 0.0, m::Int = min(10, size(A, 1)), tol::Real = 1.0e-7, opnorm = nothing, iop::Int = 0,
                        correct::Bool = false, caches = nothing, adaptive = false, delta::Real = 1.2,
                        ishermitian::Bool = LinearAlgebra.ishermitian(A), gamma::Real = 0.8, NA::Int = 0,
                        verbose = false) where {R <: MIReal, tType <: Real}
    length(ts) == ncols(U) || throw(AssertionError("Dimension mismatch"))
    (size(U, 1) == size(A, 1) == size(B, 1)) || throw(AssertionError("Dimension mismatch"))
    tsv = ts isa Vector{Float64} ? ts : Vector{Float64}(ts)
    has_opn, opn = 0, 0.0
    if opnorm !== nothing
        has_opn, opn = 1, Float64(opnorm isa Number ? opnorm : opnorm(A, Inf))
    end
    o = Ref(TimestepOpts(tau, tol, delta, gamma, opn, has_opn, m, iop, correct, adaptive, ishermitian, verbose, 0, 0, 0, NA,
                         verbose ? println_ptr() : warn_ptr(), C_NULL))
    st = Ref(TimestepStats(0, 0, 0, 0, 0, 0))
    check(ccall((:expv_mi_phiv_timestep_realop, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Int64, Cint,
                 Ref{TimestepOpts}, Ptr{Cvoid}, Ref{TimestepStats}),
                ctx().h, A.h, length(tsv), tsv, B.ptr, ld(B), ncols(B), DEVICE, U.ptr, ld(U), DEVICE, o,
                caches === nothing ? C_NULL : caches.h, st), ctx().h)
    tsv === ts || copyto!(ts, tsv)
    U
end
function phiv_timestep!(u::MIVector{Complex{R}}, t::Real, A::MIOperator{R}, B::MIMatrix{Complex{R}}; caches = nothing, kwargs...) where {R <: MIReal}
    phiv_timestep!(u, _singleton_ts(caches, t), A, B; caches = caches, kwargs...)
    u
end
function expv_timestep!(u::MIVector{Complex{R}}, t::Real, A::MIOperator{R}, b::MIVector{Complex{R}}; caches = nothing, kwargs...) where {R <: MIReal}
    phiv_timestep!(u, _singleton_ts(caches, t), A, b; caches = caches, kwargs...)
    u
end
expv_timestep!(U::MIMatrix{Complex{R}}, ts::AbstractVector{<:Real}, A::MIOperator{R}, b::MIVector{Complex{R}}; kwargs...) where {R <: MIReal} =
    phiv_timestep!(U, ts, A, b; kwargs...)

# ---- kiops(tau_out, A, u; ...)                                                                      (src/kiops.jl:57-281) ----
# Returns (w, stats) like the reference: w is n x size(tau_out, 2) (= n x 1: the only reachable case, see DESIGN.md),
# stats = (step, reject, krystep, exps, m).  The reference is real-only (kiops.jl:89, arnoldi.jl:197-200); a ComplexF64
# operator runs the documented mathematical extension.
function kiops(tau_out, A::MIOperator{T}, u::MIVecOrMat{T}; mmin::Int = 10, mmax::Int = 128, m::Int = min(mmin, mmax),
               tol::Real = 1.0e-7, opnorm = nothing, iop::Int = 2, ishermitian::Bool = LinearAlgebra.ishermitian(A),
               task1::Bool = false) where {T}
    taus = Float64.(vec(collect(tau_out)))                                    # linear indexing (kiops.jl:248)
    w = MIArray{T}(undef, size(A, 1), 1)
    o = Ref(KiopsOpts(mmin, mmax, m, iop, ishermitian, task1, 0, 0, tol))
    st = zeros(Int64, 5)
    check(ccall((:expv_mi_kiops, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cint, Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cvoid}, Int64, Cint,
                 Ref{KiopsOpts}, Ptr{Int64}),
                ctx().h, A.h, taus, length(taus), size(tau_out, 2), u.ptr, ld(u), ncols(u), DEVICE, w.ptr, ld(w), DEVICE, o, st), ctx().h)
    w, (st[1], st[2], st[3], st[4], st[5])
end

# ---- batch of independent problems over the GPUs of a node (BASELINE config 5; no reference counterpart: a host `for`) ----
# vals: nnz x nprob (values of problem p in column p, CSR order of `pattern`), B and the result: n x nprob host matrices.
function expv_batch(ts::Vector{Float64}, pattern::SparseMatrixCSC, vals::Matrix{T}, B::Matrix{T}; devices = [0],
                    m::Int = 30, tol::Real = 1.0e-7, iop::Int = 0, ishermitian::Bool = false) where {T <: MIScalar}
    P = SparseMatrixCSC(transpose(pattern))                                   # CSR of `pattern` = CSC of its transpose
    n, nprob = size(pattern, 1), size(B, 2)
    rowptr = Int32.(P.colptr .- 1)
    colind = Int32.(P.rowval .- 1)
    ctxs = [Ctx(d) for d in devices]
    W = Matrix{T}(undef, n, nprob)
    mused = zeros(Int32, nprob)
    hs = [c.h for c in ctxs]
    code = ccall((:expv_mi_expv_batch_multi, lib), Cint,
                 (Ptr{Ptr{Cvoid}}, Cint, Cint, Int64, Cint, Ptr{Int32}, Ptr{Int32}, Ptr{T}, Int64, Ptr{Cdouble}, Ptr{T}, Int64,
                  Ptr{T}, Int64, Cint, Ref{ArnoldiOpts}, Ptr{Int32}),
                 hs, length(hs), dtype(T), n, nprob, rowptr, colind, vals, size(vals, 1), ts, B, n, W, n, HOST,
                 opts(m, tol, iop, 0, ishermitian), mused)
    code == 0 || foreach(c -> check(code, c.h), ctxs)
    W, mused
end

# ---- the same batch with ONE Julia process per GPU: the final gather over RCCL (north_star: "RCCL over xGMI for the final gather only") ----
# Each process solves its contiguous block with `expv_batch(...; devices = [local_gpu])`-style calls or its own loop, leaves the block in an
# MIArray, and `allgather_columns!` brings the n x nprob result to every rank: one ncclAllGather on the context's stream.  The 128-byte id comes
# from rank 0 (`rccl_unique_id()`) and reaches the other ranks by the host's own means (MPI.jl bcast, Distributed.jl, a file).
rccl_available() = ccall((:expv_mi_rccl_available, lib), Cint, ()) == 1
function rccl_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:expv_mi_rccl_unique_id, lib), Cint, (Ptr{UInt8},), id), C_NULL)
    id
end
mutable struct RcclComm
    h::Ptr{Cvoid}
    nranks::Int
    rank::Int
    function RcclComm(id::Vector{UInt8}, nranks::Integer, rank::Integer)
        length(id) == 128 || throw(ArgumentError("unique id: 128 bytes"))
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:expv_mi_comm_create, lib), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint, Ptr{Ptr{Cvoid}}), ctx().h, id, nranks, rank, h), ctx().h)
        c = new(h[], nranks, rank)
        finalizer(x -> ccall((:expv_mi_comm_destroy, lib), Cint, (Ptr{Cvoid},), x.h), c)
        c
    end
end
# recv[:, r * cols + 1 : (r + 1) * cols] = rank r's `send` (n x cols, contiguous): the blocks of `dist.shard_range` with equal shares
function allgather_columns!(recv::MIArray{T}, send::MIArray{T}, comm::RcclComm) where {T}
    length(recv) == comm.nranks * length(send) || throw(DimensionMismatch("recv must hold nranks blocks of send's size"))
    check(ccall((:expv_mi_gather_rccl, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint),
                comm.h, send.ptr, recv.ptr, length(send), dtype(T)), ctx().h)
    recv
end

end # module
