// sparse_rows.h -- the rows of a stored sparse operator applied to a vector, one 16-byte row pack per lane (gfx950 only):
// from the SELL-C slots or from the general DIA form.  Shared by the Krylov half-steps (fused.hip) and the truncated-Taylor term
// kernels (expv_taylor.hip: one vector; expv_taylor_block.hip and the norm estimator's panel kernel, op_normest.hip: P interleaved
// columns behind the same two loops).
#pragma once
#include "kernel_common.h"

namespace expv_mi {
namespace dev {

template <class T>
__device__ __forceinline__ void load_cols(const int32_t *p, int32_t *c);
template <>
__device__ __forceinline__ void load_cols<double>(const int32_t *p, int32_t *c) {
  const int2 v = *reinterpret_cast<const int2 *>(p);
  c[0] = v.x;
  c[1] = v.y;
}
template <>
__device__ __forceinline__ void load_cols<cplx>(const int32_t *p, int32_t *c) { c[0] = *p; }
template <>
__device__ __forceinline__ void load_cols<float>(const int32_t *p, int32_t *c) {      // 4 rows per lane
  const int4 v = *reinterpret_cast<const int4 *>(p);
  c[0] = v.x;
  c[1] = v.y;
  c[2] = v.z;
  c[3] = v.w;
}
template <>
__device__ __forceinline__ void load_cols<cplx32>(const int32_t *p, int32_t *c) {
  const int2 v = *reinterpret_cast<const int2 *>(p);
  c[0] = v.x;
  c[1] = v.y;
}

// The two operator loops below are written once for whatever stands on the right-hand side.  X is the operand and the accumulator
// of a lane's N rows:
//   typename X::row_t        what one column index fetches (one element of a vector; the P adjacent values of an interleaved block)
//   x.clear(k)               acc_k = 0
//   x.at(c) / X::none()      the operand of column c / of a column outside the matrix
//   x.fma(k, a, g)           acc_k += a * g, one ST<T>::fma_ per accumulated value
// OneVector is the single right-hand side of dia_rows / sell_rows.  Q = the diagonals / slots a lane keeps in flight; the sums run in
// ascending order whatever Q is.
template <class T>
struct OneVector {
  using row_t = T;
  const T *__restrict__ x;
  T *acc;
  __device__ __forceinline__ void clear(int k) { acc[k] = ST<T>::zero(); }
  __device__ __forceinline__ T at(int64_t c) const { return x[c]; }
  __device__ __forceinline__ static T none() { return ST<T>::zero(); }
  __device__ __forceinline__ void fma(int k, T a, const T &g) { ST<T>::fma_(acc[k], a, g); }
};

// one row of an interleaved work vector: the P values of a row, adjacent and 16-byte aligned
template <class T, int P>
struct __attribute__((aligned(16))) RowP {
  static_assert(P * sizeof(T) % 16 == 0, "a row of the interleaved work vectors is a whole number of 16-byte packs");
  T v[P];
};

// the right-hand side of the operator loops of sparse_rows.h: P columns at once
template <class T, int P>
struct BlockColumns {
  using row_t = RowP<T, P>;
  const T *__restrict__ x;
  T (*acc)[P];
  __device__ __forceinline__ void clear(int k) {
#pragma unroll
    for (int p = 0; p < P; ++p) acc[k][p] = ST<T>::zero();
  }
  __device__ __forceinline__ row_t at(int64_t c) const { return *reinterpret_cast<const row_t *>(x + c * P); }
  __device__ __forceinline__ static row_t none() {
    row_t r;
#pragma unroll
    for (int p = 0; p < P; ++p) r.v[p] = ST<T>::zero();
    return r;
  }
  __device__ __forceinline__ void fma(int k, T a, const row_t &g) {
#pragma unroll
    for (int p = 0; p < P; ++p) ST<T>::fma_(acc[k][p], a, g.v[p]);
  }
};

// y-rows of one slice for this lane from the DIA form: acc[k] = sum_d val[d][r] * x[r + off[d]]  (ascending offsets =
// ascending columns: the order of the CSR/SELL row; absent entries are explicit zeros)
template <class T, int Q, class X>
__device__ __forceinline__ void dia_walk(const T *__restrict__ dval, int64_t ld, int ndiag, const int32_t *__restrict__ doff,
                                         int64_t i, int64_t n, X &xs) {
  constexpr int N = Pack<T>::N;
  using R = typename X::row_t;
#pragma unroll
  for (int k = 0; k < N; ++k) xs.clear(k);
  int d = 0;
  for (; d + Q <= ndiag; d += Q) {   // Q diagonals in flight
    Pack<T> v[Q];
    R xv[Q][N];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      v[q] = *reinterpret_cast<const Pack<T> *>(dval + (int64_t)(d + q) * ld + i);
      const int64_t c0 = i + doff[d + q];
#pragma unroll
      for (int k = 0; k < N; ++k) xv[q][k] = (c0 + k >= 0 && c0 + k < n) ? xs.at(c0 + k) : X::none();
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) xs.fma(k, v[q].v[k], xv[q][k]);
  }
  for (; d < ndiag; ++d) {
    const Pack<T> v = *reinterpret_cast<const Pack<T> *>(dval + (int64_t)d * ld + i);
    const int64_t c0 = i + doff[d];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const R xk = (c0 + k >= 0 && c0 + k < n) ? xs.at(c0 + k) : X::none();
      xs.fma(k, v.v[k], xk);
    }
  }
}
template <class T>
__device__ __forceinline__ void dia_rows(const T *__restrict__ dval, int64_t ld, int ndiag, const int32_t *__restrict__ doff,
                                         int64_t i, int64_t n, const T *__restrict__ x, T *acc) {
  OneVector<T> xs{x, acc};
  dia_walk<T, 4>(dval, ld, ndiag, doff, i, n, xs);
}

// y-rows of one slice for this lane: acc[k] = sum_slots val * x[col]
template <class T, int Q, class X>
__device__ __forceinline__ void sell_walk(const SellView<T> &A, int64_t slice, int lane, X &xs) {
  constexpr int N = Pack<T>::N;
  constexpr int SH = 64 * N;
  using R = typename X::row_t;
  const int64_t off = A.slice_off[slice];
  const int L = (int)((A.slice_off[slice + 1] - off) / SH);
  const T *vp = A.val + off + (int64_t)lane * N;
  const int32_t *cp = A.col + off + (int64_t)lane * N;
#pragma unroll
  for (int k = 0; k < N; ++k) xs.clear(k);
  int s = 0;
  for (; s + Q <= L; s += Q) {  // Q slots in flight: Q x 16 B of values + indices, then Q N gathers
    Pack<T> v[Q];
    int32_t c[Q][N];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      v[q] = *reinterpret_cast<const Pack<T> *>(vp + (int64_t)(s + q) * SH);
      load_cols<T>(cp + (int64_t)(s + q) * SH, c[q]);
    }
    R xv[Q][N];
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) xv[q][k] = xs.at(c[q][k]);
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) xs.fma(k, v[q].v[k], xv[q][k]);
  }
  for (; s < L; ++s) {
    const Pack<T> v = *reinterpret_cast<const Pack<T> *>(vp + (int64_t)s * SH);
    int32_t c[N];
    load_cols<T>(cp + (int64_t)s * SH, c);
#pragma unroll
    for (int k = 0; k < N; ++k) xs.fma(k, v.v[k], xs.at(c[k]));
  }
}
template <class T>
__device__ __forceinline__ void sell_rows(const SellView<T> &A, int64_t slice, int lane, const T *__restrict__ x,
                                          T *acc) {
  OneVector<T> xs{x, acc};
  sell_walk<T, 4>(A, slice, lane, xs);
}

}  // namespace dev
}  // namespace expv_mi
