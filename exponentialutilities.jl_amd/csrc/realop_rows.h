// realop_rows.h -- a REAL stored operator applied to COMPLEX vectors (gfx950 only): what the truncated-Taylor series for a real
// operator (expv_taylor_realop.hip) and the Krylov step of a mixed call (krylov_realop.hip) share.  The operator is read in its own
// real type R, the vectors have its complex counterpart C: a complex vector of n elements is an interleaved real block of n x 2, so
// (A x)_i is the block product of sparse_rows.h with a row of one C.
#pragma once
#include "kernel_common.h"
#include "sparse_rows.h"

namespace expv_mi {
namespace dev {

template <class R> struct ComplexOf;
template <> struct ComplexOf<double> { using type = cplx; };
template <> struct ComplexOf<float> { using type = cplx32; };

// The right-hand side of the operator loops of sparse_rows.h for a real operator on a complex vector: BlockColumns<R, 2> on the
// interleaved (re, im) pairs -- acc.re = fma(a, x.re, acc.re), acc.im = fma(a, x.im, acc.im), one ST<R>::fma_ per component -- with
// one C as the row (16 bytes in ComplexF64, 8 in ComplexF32, which RowP's whole-pack rule leaves out).
template <class R>
struct RealOnComplex {
  using C = typename ComplexOf<R>::type;
  using row_t = C;
  const C *__restrict__ x;
  R (*acc)[2];
  __device__ __forceinline__ void clear(int k) { acc[k][0] = ST<R>::zero(); acc[k][1] = ST<R>::zero(); }
  __device__ __forceinline__ C at(int64_t c) const { return x[c]; }
  __device__ __forceinline__ static C none() { return ST<C>::zero(); }
  __device__ __forceinline__ void fma(int k, R a, const C &g) {
    ST<R>::fma_(acc[k][0], a, g.re);
    ST<R>::fma_(acc[k][1], a, g.im);
  }
};

// The Pack<R>::N rows of a lane as complex elements: 32 contiguous bytes, two 16-byte accesses (a wave covers 2 KB or 4 KB in one
// piece).  The vectors hold exactly n elements: the last pack goes element by element.
template <class C>
struct CRows { Pack<C> h[2]; };
template <class C>
__device__ __forceinline__ CRows<C> ld_crows(const C *__restrict__ p, int64_t i, int64_t n, bool al) {
  CRows<C> r;
  r.h[0] = ld_pack_user(p, i, n, al);
  r.h[1] = ld_pack_user(p, i + Pack<C>::N, n, al);
  return r;
}
template <class C>
__device__ __forceinline__ void st_crows(C *__restrict__ p, int64_t i, int64_t n, bool al, const CRows<C> &r) {
  st_pack_user(p, i, n, al, r.h[0]);
  st_pack_user(p, i + Pack<C>::N, n, al, r.h[1]);
}

// z = (x, +0): a real b in the complex type.  x and z do not overlap.
template <class R>
__global__ __launch_bounds__(BLOCK) void k_realop_widen(const R *__restrict__ x, typename ComplexOf<R>::type *__restrict__ z, int64_t n) {
  using C = typename ComplexOf<R>::type;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    C v;
    v.re = x[i];
    v.im = ST<R>::zero();
    z[i] = v;
  }
}
// the planes of a complex vector (path 2: the v a closing launch left)
template <class R>
__global__ __launch_bounds__(BLOCK) void k_realop_planes(const typename ComplexOf<R>::type *__restrict__ z, R *__restrict__ re, R *__restrict__ im, int64_t n) {
  using C = typename ComplexOf<R>::type;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    const C v = z[i];
    re[i] = v.re;
    im[i] = v.im;
  }
}

}  // namespace dev
}  // namespace expv_mi
