// op_lincomb.hip -- the operator C = c_1 A_1 + ... + c_K A_K (+ c_I I) of operators that exist, K <= LINCOMB_MAX_TERMS, made on the
// device from the arrays the terms store (capi.hip: expv_mi_op_create_lincomb, expv_mi_op_lincomb_refresh).  Neither the terms'
// values nor the combined ones visit the host.
//
// Sparse terms.  A term stores CSR32 arrays rowptr / col / val, in its own row ordering when it was reordered (stored as P A P';
// p[i] = natural row at position i).  C is DEFINED as the operator expv_mi_op_create_csr_loc makes of zero-based CSR32 arrays in
// the natural ordering whose pattern is the union of the terms' coordinates (and the diagonal, with the identity), every row in
// strictly ascending column order, so this file and op_coo.hip produce exactly those arrays:
//   1. k_lc_key       one launch per term over its stored entries, four per thread: the row of an entry by bisection on rowptr
//                     (as k_adj_key of op_adjoint.hip does), relabelled through p, the 64-bit key  p[row] << 32 | p[col]  and as
//                     payload the entry's position in the CONCATENATION of the terms' stored arrays, term after term;
//      k_lc_ident     the identity's n entries  i << 32 | i  behind them.
//   2. dev::coo_sort (stable), coo_count_heads and coo_compress of op_coo.hip, as they are: the sorted payload is the map src,
//      the heads give rowptr / colind and the segment table seg.  Inside a segment the positions ascend -- the sort is stable --
//      so its entries stand in term order, inside a term in the term's stored order, the identity last.
//   3. k_lc_gather    out[e] = the contributions of segment e added left to right, the accumulator STARTING as the first one (a
//                     lone -0 survives): creation and every refresh, the hot path.  A lane owns one 16-byte pack of the result
//                     and walks the segments of its entries; the term of a position comes from at most 8 compares against
//                     offsets held in the kernel arguments, and its value pointer and coefficient are selected from there too.
// The roundings are the contract (include/expv_mi.h): a real coefficient multiplies each real component once; a complex one gives
// (cr ar - ci ai, cr ai + ci ar), every product rounded, then the sum or difference rounded; the identity contributes its
// coefficient as it is.  Every such operation stands under `fp contract(off)`: nothing is fused.  No floating-point atomic is
// used anywhere, so two creations -- and a creation and a refresh -- give the same bits.
//
// Dense terms.  k_lc_dense writes the packed (leading dimension n) column-major matrix of the combination: a lane owns one pack of
// consecutive rows of a column, reads the pack of every term with one 16-byte load where it lies inside the matrix and its address
// is 16-byte aligned (single components otherwise: a caller's array is aligned to its real type at least) and adds in term order,
// the identity last and on the diagonal only.  Rows n .. lda - 1 of a term are never read: every load is guarded by i < n.
//
// Unchecked values: none are indexed by.  rowptr / col / p of a term are arrays the library built and checked at the term's creation
// (col in [0, n), p a permutation of [0, n), rowptr non-decreasing from 0 to nnz); src is the sort's payload, a permutation of the
// positions [0, sum nnz_k (+ n)), so src[q] - off[t] lies in [0, nnz_t); seg is the head table coo_compress wrote, ascending from 0
// to that same total.  Memory: no LDS, no scratch (the term table is read from the kernel arguments).
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"
#include "op_lincomb.h"

namespace expv_mi {
namespace dev {

namespace {
typedef unsigned long long ull;
constexpr int LC_KEY_TILE = 4096;                   // stored entries a workgroup of k_lc_key relabels
static_assert(LC_KEY_TILE % (BLOCK * 4) == 0, "whole trips of four entries per thread");

template <class T> struct alignas(16) LcPack { T v[16 / sizeof(T)]; };

// the i in [lo, hi] with ptr[i] <= e < ptr[i + 1]; the caller knows that there is one
__device__ __forceinline__ int64_t lc_find_row(const int32_t *__restrict__ ptr, int64_t lo, int64_t hi, int32_t e) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid + 1] > e) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(BLOCK) void k_lc_key(const int32_t *__restrict__ ptr, const int32_t *__restrict__ col, const int32_t *__restrict__ p,
                                                  int64_t n, int64_t nnz, int64_t base, ull *__restrict__ key, int32_t *__restrict__ pay) {
  const int64_t e0 = (int64_t)blockIdx.x * LC_KEY_TILE, eend = e0 + LC_KEY_TILE < nnz ? e0 + LC_KEY_TILE : nnz;
  const int64_t rlo = lc_find_row(ptr, 0, n - 1, (int32_t)e0), rhi = lc_find_row(ptr, rlo, n - 1, (int32_t)(eend - 1));
  for (int64_t e = e0 + (int64_t)threadIdx.x * 4; e < eend; e += BLOCK * 4) {
    const int len = eend - e >= 4 ? 4 : (int)(eend - e);
    int64_t i = lc_find_row(ptr, rlo, rhi, (int32_t)e);
    int32_t next = ptr[i + 1];
#pragma unroll
    for (int z = 0; z < 4; ++z)
      if (z < len) {
        while ((int32_t)(e + z) >= next) { ++i; next = ptr[i + 1]; }      // (a later row stores entry e + z: e + z < nnz)
        const int32_t c = col[e + z];
        const uint32_t r2 = (uint32_t)(p ? p[i] : (int32_t)i), c2 = (uint32_t)(p ? p[c] : c);
        key[base + e + z] = ((ull)r2 << 32) | (ull)c2;      // (base is any count of entries: single stores)
        pay[base + e + z] = (int32_t)(base + e + z);
      }
  }
}

__global__ __launch_bounds__(BLOCK) void k_lc_ident(int64_t n, int64_t base, ull *__restrict__ key, int32_t *__restrict__ pay) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    key[base + i] = ((ull)(uint32_t)i << 32) | (ull)(uint32_t)i;
    pay[base + i] = (int32_t)(base + i);
  }
}

// ---- the roundings of one contribution and of one addition, by definition ----
template <class T>
__device__ __forceinline__ T lc_scale(typename ST<T>::real_t cr, typename ST<T>::real_t ci, T a) {
#pragma clang fp contract(off)
  if constexpr (ST<T>::is_complex) {
    using R = typename ST<T>::real_t;
    T y;
    if (ci == (R)0) {
      y.re = cr * a.re;
      y.im = cr * a.im;
    } else {
      const R p1 = cr * a.re, p2 = ci * a.im, p3 = cr * a.im, p4 = ci * a.re;
      y.re = p1 - p2;
      y.im = p3 + p4;
    }
    return y;
  } else {
    return cr * a;
  }
}
template <class T>
__device__ __forceinline__ T lc_add(T a, T b) {
#pragma clang fp contract(off)
  if constexpr (ST<T>::is_complex) {
    a.re = a.re + b.re;
    a.im = a.im + b.im;
    return a;
  } else {
    return a + b;
  }
}
template <class T>
__device__ __forceinline__ T lc_identity(const LincombTerms<T> &a) {
  if constexpr (ST<T>::is_complex) {
    T y;
    y.re = a.cre[a.nterms];
    y.im = a.cim[a.nterms];
    return y;
  } else {
    return a.cre[a.nterms];
  }
}
// a value of a caller's array, aligned to its real type at least: read by its components
template <class T> __device__ __forceinline__ T lc_load_parts(const T *p) {
  using R = typename ST<T>::real_t;
  const R *r = reinterpret_cast<const R *>(p);
  T v;
  if constexpr (ST<T>::is_complex) { v.re = r[0]; v.im = r[1]; }
  else v = r[0];
  return v;
}

// the contribution of position g of the concatenation
template <class T>
__device__ __forceinline__ T lc_contribution(const LincombTerms<T> &a, int32_t g) {
  using R = typename ST<T>::real_t;
  if (g >= a.off[a.nterms]) return lc_identity(a);      // (positions from off[nterms] on exist with the identity only)
  // The term's slot of the table by selects between values that are the same in every lane: constant indices, so the table is read
  // by scalar loads, once per wave.  (Indexing it by the lane's own term number would be a vector load from the kernel-argument
  // segment for every contribution.)  off[k] = INT32_MAX > g beyond the terms.
  const T *v = a.val[0];
  int32_t o = a.off[0];
  R cr = a.cre[0], ci = a.cim[0];
#pragma unroll
  for (int k = 1; k < LINCOMB_MAX_TERMS; ++k) {
    const bool later = g >= a.off[k];
    v = later ? a.val[k] : v;
    o = later ? a.off[k] : o;
    cr = later ? a.cre[k] : cr;
    ci = later ? a.cim[k] : ci;
  }
  return lc_scale<T>(cr, ci, v[g - o]);
}

template <class T>
__global__ __launch_bounds__(BLOCK) void k_lc_gather(const LincombTerms<T> a, const int32_t *__restrict__ src, const int32_t *__restrict__ seg,
                                                     int64_t nstored, T *__restrict__ out) {
  constexpr int VPT = 16 / (int)sizeof(T);
  for (int64_t e = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * VPT; e < nstored; e += (int64_t)gridDim.x * BLOCK * VPT) {
    const int len = nstored - e >= VPT ? VPT : (int)(nstored - e);
    LcPack<T> v;
    int32_t s0 = seg[e];
#pragma unroll
    for (int z = 0; z < VPT; ++z)
      if (z < len) {
        const int32_t s1 = seg[e + z + 1];      // (seg has nstored + 1 words; s1 > s0: a stored entry has one position at least)
        T acc = lc_contribution(a, src[s0]);
        for (int32_t q = s0 + 1; q < s1; ++q) acc = lc_add(acc, lc_contribution(a, src[q]));
        v.v[z] = acc;
        s0 = s1;
      }
    if (len == VPT) *reinterpret_cast<LcPack<T> *>(out + e) = v;      // (out: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)      // (constant indices: the pack stays in registers)
        if (z < len) out[e + z] = v.v[z];
    }
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void k_lc_dense(const LincombTerms<T> a, int64_t n, int64_t ch, T *__restrict__ out) {
  constexpr int VPT = 16 / (int)sizeof(T);
  const int64_t total = ch * n;      // packs of a column x columns
  for (int64_t w = (int64_t)blockIdx.x * BLOCK + threadIdx.x; w < total; w += (int64_t)gridDim.x * BLOCK) {
    const int64_t j = w / ch, i = (w - j * ch) * VPT;
    const int len = n - i >= VPT ? VPT : (int)(n - i);
    LcPack<T> acc;
    for (int k = 0; k < a.nterms; ++k) {      // (the same k in every lane: the term table is read by scalar loads)
      const T *from = a.val[k] + j * a.lda[k] + i;
      LcPack<T> v;
      if (len == VPT && (reinterpret_cast<uintptr_t>(from) & 15u) == 0) v = *reinterpret_cast<const LcPack<T> *>(from);
      else {
#pragma unroll
        for (int z = 0; z < VPT; ++z)
          if (z < len) v.v[z] = lc_load_parts(from + z);
      }
#pragma unroll
      for (int z = 0; z < VPT; ++z)
        if (z < len) {
          const T c = lc_scale<T>(a.cre[k], a.cim[k], v.v[z]);
          acc.v[z] = k == 0 ? c : lc_add(acc.v[z], c);
        }
    }
    if (a.identity) {
#pragma unroll
      for (int z = 0; z < VPT; ++z)
        if (z < len && i + z == j) acc.v[z] = lc_add(acc.v[z], lc_identity(a));
    }
    T *to = out + j * n + i;
    if (len == VPT && (reinterpret_cast<uintptr_t>(to) & 15u) == 0) *reinterpret_cast<LcPack<T> *>(to) = acc;
    else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)
        if (z < len) to[z] = acc.v[z];
    }
  }
}

void check_launch(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + hipGetErrorString(e));
}

template <class T>
void check_terms(const LincombTerms<T> &a, const char *who) {
  if (a.nterms < 1 || a.nterms > LINCOMB_MAX_TERMS) throw std::runtime_error(std::string(who) + ": bad number of terms");
  for (int k = 0; k < a.nterms; ++k)
    if (!a.val[k]) throw std::runtime_error(std::string(who) + ": null values of a term");
}
}  // namespace

int lincomb_pack(int value_bytes) { return 16 / value_bytes; }

void lincomb_keys(hipStream_t s, const int32_t *rowptr, const int32_t *col, const int32_t *p, int64_t n, int64_t nnz, int64_t base,
                  unsigned long long *key, int32_t *pay) {
  if (n < 0 || nnz < 0 || base < 0 || n > 0x7fffffffLL || base + nnz > 0x7fffffffLL) throw std::runtime_error("lincomb_keys: bad sizes");
  if (nnz == 0) return;
  hipLaunchKernelGGL(k_lc_key, dim3((unsigned)((nnz + LC_KEY_TILE - 1) / LC_KEY_TILE)), dim3(BLOCK), 0, s, rowptr, col, p, n, nnz, base, key, pay);
  check_launch("lincomb_keys");
}

void lincomb_identity_keys(hipStream_t s, int64_t n, int64_t base, unsigned long long *key, int32_t *pay) {
  if (n < 0 || base < 0 || base + n > 0x7fffffffLL) throw std::runtime_error("lincomb_identity_keys: bad sizes");
  if (n == 0) return;
  hipLaunchKernelGGL(k_lc_ident, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, s, n, base, key, pay);
  check_launch("lincomb_identity_keys");
}

template <class T>
void lincomb_gather(hipStream_t s, const LincombTerms<T> &a, const int32_t *src, const int32_t *seg, int64_t nstored, T *out) {
  if (nstored < 0 || nstored > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
    throw std::runtime_error("lincomb_gather: bad nnz / output alignment");
  if (a.nterms < 0 || a.nterms > LINCOMB_MAX_TERMS) throw std::runtime_error("lincomb_gather: bad number of terms");
  if (nstored == 0) return;
  for (int k = 0; k < a.nterms; ++k)      // (a term without entries is never read)
    if (!a.val[k] && a.off[k + 1] > a.off[k]) throw std::runtime_error("lincomb_gather: null values of a term");
  hipLaunchKernelGGL(k_lc_gather<T>, dim3(grid_for(nstored, BLOCK * (16 / (int)sizeof(T)))), dim3(BLOCK), 0, s, a, src, seg, nstored, out);
  check_launch("lincomb_gather");
}
template void lincomb_gather<double>(hipStream_t, const LincombTerms<double> &, const int32_t *, const int32_t *, int64_t, double *);
template void lincomb_gather<cplx>(hipStream_t, const LincombTerms<cplx> &, const int32_t *, const int32_t *, int64_t, cplx *);
template void lincomb_gather<float>(hipStream_t, const LincombTerms<float> &, const int32_t *, const int32_t *, int64_t, float *);
template void lincomb_gather<cplx32>(hipStream_t, const LincombTerms<cplx32> &, const int32_t *, const int32_t *, int64_t, cplx32 *);

template <class T>
void lincomb_dense(hipStream_t s, const LincombTerms<T> &a, int64_t n, T *out) {
  if (n < 0) throw std::runtime_error("lincomb_dense: bad n");
  if (n == 0) return;
  check_terms(a, "lincomb_dense");
  for (int k = 0; k < a.nterms; ++k)
    if (a.lda[k] < n) throw std::runtime_error("lincomb_dense: bad lda");
  constexpr int VPT = 16 / (int)sizeof(T);
  const int64_t ch = (n + VPT - 1) / VPT;
  hipLaunchKernelGGL(k_lc_dense<T>, dim3(grid_for(ch * n, BLOCK)), dim3(BLOCK), 0, s, a, n, ch, out);
  check_launch("lincomb_dense");
}
template void lincomb_dense<double>(hipStream_t, const LincombTerms<double> &, int64_t, double *);
template void lincomb_dense<cplx>(hipStream_t, const LincombTerms<cplx> &, int64_t, cplx *);
template void lincomb_dense<float>(hipStream_t, const LincombTerms<float> &, int64_t, float *);
template void lincomb_dense<cplx32>(hipStream_t, const LincombTerms<cplx32> &, int64_t, cplx32 *);

}  // namespace dev
}  // namespace expv_mi
