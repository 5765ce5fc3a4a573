// sparse_rows.h -- the rows of a stored sparse operator applied to a vector, one 16-byte row pack per lane (gfx950 only):
// from the SELL-C slots or from the general DIA form.  Shared by the Krylov half-steps (fused.hip) and the truncated-Taylor term
// kernel (expv_taylor.hip).
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

// y-rows of one slice for this lane from the DIA form: acc[k] = sum_d val[d][r] * x[r + off[d]]  (ascending offsets =
// ascending columns: the order of the CSR/SELL row; absent entries are explicit zeros)
template <class T>
__device__ __forceinline__ void dia_rows(const T *__restrict__ dval, int64_t ld, int ndiag, const int32_t *__restrict__ doff,
                                         int64_t i, int64_t n, const T *__restrict__ x, T *acc) {
  constexpr int N = Pack<T>::N;
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = ST<T>::zero();
  int d = 0;
  for (; d + 4 <= ndiag; d += 4) {   // 4 diagonals in flight
    Pack<T> v[4];
    T xv[4][N];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = *reinterpret_cast<const Pack<T> *>(dval + (int64_t)(d + q) * ld + i);
      const int64_t c0 = i + doff[d + q];
#pragma unroll
      for (int k = 0; k < N; ++k) xv[q][k] = (c0 + k >= 0 && c0 + k < n) ? x[c0 + k] : ST<T>::zero();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) ST<T>::fma_(acc[k], v[q].v[k], xv[q][k]);
  }
  for (; d < ndiag; ++d) {
    const Pack<T> v = *reinterpret_cast<const Pack<T> *>(dval + (int64_t)d * ld + i);
    const int64_t c0 = i + doff[d];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const T xk = (c0 + k >= 0 && c0 + k < n) ? x[c0 + k] : ST<T>::zero();
      ST<T>::fma_(acc[k], v.v[k], xk);
    }
  }
}

// y-rows of one slice for this lane: acc[k] = sum_slots val * x[col]
template <class T>
__device__ __forceinline__ void sell_rows(const SellView<T> &A, int64_t slice, int lane, const T *__restrict__ x,
                                          T *acc) {
  constexpr int N = Pack<T>::N;
  constexpr int SH = 64 * N;
  const int64_t off = A.slice_off[slice];
  const int L = (int)((A.slice_off[slice + 1] - off) / SH);
  const T *vp = A.val + off + (int64_t)lane * N;
  const int32_t *cp = A.col + off + (int64_t)lane * N;
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = ST<T>::zero();
  int s = 0;
  for (; s + 4 <= L; s += 4) {  // 4 slots in flight: 4 x 16 B of values + indices, then 4N gathers
    Pack<T> v[4];
    int32_t c[4][N];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = *reinterpret_cast<const Pack<T> *>(vp + (int64_t)(s + q) * SH);
      load_cols<T>(cp + (int64_t)(s + q) * SH, c[q]);
    }
    T xv[4][N];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) xv[q][k] = x[c[q][k]];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < N; ++k) ST<T>::fma_(acc[k], v[q].v[k], xv[q][k]);
  }
  for (; s < L; ++s) {
    const Pack<T> v = *reinterpret_cast<const Pack<T> *>(vp + (int64_t)s * SH);
    int32_t c[N];
    load_cols<T>(cp + (int64_t)s * SH, c);
#pragma unroll
    for (int k = 0; k < N; ++k) ST<T>::fma_(acc[k], v.v[k], x[c[k]]);
  }
}

}  // namespace dev
}  // namespace expv_mi
