// op_adjoint.hip -- the operator of A' = conj(transpose(A)) or of transpose(A), made on the device from the arrays an existing
// operator stores (capi.hip: create_adjoint, expv_mi_op_adjoint_refresh).  Neither the parent's values nor their transposed copies
// visit the host.
//
// Sparse parents.  The parent stores CSR32 arrays rowptr / col / val, in its own row ordering when it was reordered (stored as
// P A P'; p[i] = natural row at position i).  The adjoint is DEFINED as the operator expv_mi_op_create_csr_loc makes of the
// zero-based CSR32 arrays of the transpose in the natural ordering, every row in ascending column order, so this file produces
// exactly those arrays:
//   1. k_adj_key      one streaming pass over the stored entries, four per thread: the row of an entry by bisection on rowptr
//                     (first for the two ends of the workgroup's tile, then per thread inside that range; the following entries by
//                     stepping), relabelled through p, and the 64-bit key  p[col] << 32 | p[row]  -- the entry's coordinate in the
//                     transpose -- with the entry's stored position as payload.
//   2. the stable LSD radix sort of op_coo.hip (dev::coo_sort) orders the keys; entries of one coordinate (a parent whose rows
//      repeat a column) stay separate, adjacent, in the parent's stored order: deterministic.  The payload becomes the map
//      src[e] = parent stored entry of adjoint entry e, which the operator keeps for expv_mi_op_adjoint_refresh.
//   3. k_adj_idx      idx32[e] = low word of the sorted key (16-byte stores) and the count of positions that repeat their
//                     predecessor's key (an integer count: order-free) -- zero means every row is strictly ascending;
//      k_adj_ptr      ptr32[i], i <= n, by bisection over the sorted keys' high words: one thread per ROW, so empty rows need no
//                     special case.
//   4. k_adj_gather   out[e] = op(val[src[e]]): creation and every refresh.  16-byte stores, gathers of single elements.
// Nothing here uses a floating-point atomic, and values are never added: two creations give the same bits.
//
// Dense parents.  k_adj_dense writes the packed (leading dimension n) column-major copy of op(A)'.  A workgroup owns a TILE x TILE
// tile: it reads the tile's columns -- contiguous in the parent -- with 16-byte loads where a whole pack lies inside the matrix and
// its address is 16-byte aligned (single elements otherwise), into the LDS image t[c (TILE + 1) + r], and writes the tile's rows --
// contiguous in the copy -- with 16-byte stores under the same two conditions, reading t with the roles of c and r swapped.  The
// row stride TILE + 1 is odd in elements: consecutive lanes of the transposed read are VPT (TILE + 1) elements apart (VPT the
// elements of a pack), i.e. 4 banks further on for every element size, and the lanes of the next column of the copy are shifted
// by one element.  By the bank rules (32 banks for 4-byte reads, 64 for wider ones; lanes conflict inside a 32-lane half, a 16-lane
// group for 16-byte reads) that is two-way for 4- and 8-byte elements and conflict-free for 16-byte ones, where an unpadded tile
// would put a whole half on one bank.  (Reasoned from the layout; no LDS counter was read.)  Rows n .. lda - 1 of the parent are
// never read: every load is guarded by i < n.
//
// Unchecked values: none are indexed by.  rowptr / col / p are arrays the library built and checked at the parent's creation (col in
// [0, n), p a permutation of [0, n), rowptr non-decreasing from 0 to nnz); src is the sort's payload, a permutation of [0, nnz).
// Memory: the dense tile, at most 64 x 65 x 8 = 33 280 bytes of static LDS; no scratch.
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"

namespace expv_mi {
namespace dev {

namespace {
typedef unsigned long long ull;
constexpr int ADJ_KEY_TILE = 4096;                  // stored entries a workgroup of k_adj_key relabels
constexpr int ADJ_TILE = 64;                        // side of the dense tile for 4- and 8-byte elements
constexpr int ADJ_TILE16 = 32;                      // ... and for 16-byte ones (32 x 33 x 16 bytes of LDS)
constexpr ull SIGN64 = 1ull << 63;
static_assert(ADJ_KEY_TILE % (BLOCK * 4) == 0, "whole trips of four entries per thread");

typedef ull U16 __attribute__((ext_vector_type(2), aligned(8)));      // a 16-byte element, 8-byte aligned in a caller's array
template <class U> struct alignas(16) Pack16 { U v[16 / sizeof(U)]; };

// the conjugate of a raw complex unit: (re, im) interleaved, im in the upper half
template <bool CONJ> __device__ __forceinline__ uint32_t unit_op(uint32_t v) { static_assert(!CONJ, "4-byte elements are real"); return v; }
template <bool CONJ> __device__ __forceinline__ ull unit_op(ull v) { return CONJ ? v ^ SIGN64 : v; }
template <bool CONJ> __device__ __forceinline__ U16 unit_op(U16 v) { if (CONJ) v.y ^= SIGN64; return v; }

// the i in [lo, hi] with ptr[i] <= e < ptr[i + 1]; the caller knows that there is one
__device__ __forceinline__ int64_t find_row(const int32_t *__restrict__ ptr, int64_t lo, int64_t hi, int32_t e) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid + 1] > e) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(BLOCK) void k_adj_key(const int32_t *__restrict__ ptr, const int32_t *__restrict__ col, const int32_t *__restrict__ p,
                                                   int64_t n, int64_t nnz, ull *__restrict__ key, int32_t *__restrict__ pay) {
  const int64_t e0 = (int64_t)blockIdx.x * ADJ_KEY_TILE, eend = e0 + ADJ_KEY_TILE < nnz ? e0 + ADJ_KEY_TILE : nnz;
  const int64_t rlo = find_row(ptr, 0, n - 1, (int32_t)e0), rhi = find_row(ptr, rlo, n - 1, (int32_t)(eend - 1));
  for (int64_t e = e0 + (int64_t)threadIdx.x * 4; e < eend; e += BLOCK * 4) {
    const int len = eend - e >= 4 ? 4 : (int)(eend - e);
    int64_t i = find_row(ptr, rlo, rhi, (int32_t)e);
    int32_t next = ptr[i + 1];
    ull o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int z = 0; z < 4; ++z)
      if (z < len) {
        while ((int32_t)(e + z) >= next) { ++i; next = ptr[i + 1]; }      // (a later row stores entry e + z: e + z < nnz)
        const int32_t c = col[e + z];
        const uint32_t r2 = (uint32_t)(p ? p[c] : c), c2 = (uint32_t)(p ? p[i] : (int32_t)i);
        o[z] = ((ull)r2 << 32) | (ull)c2;
      }
    if (len == 4) {      // (key, pay: the library's buffers, 16-byte aligned; e is a multiple of 4)
      ulonglong2 *k2 = reinterpret_cast<ulonglong2 *>(key + e);
      k2[0] = make_ulonglong2(o[0], o[1]);
      k2[1] = make_ulonglong2(o[2], o[3]);
      *reinterpret_cast<int4 *>(pay + e) = make_int4((int32_t)e, (int32_t)e + 1, (int32_t)e + 2, (int32_t)e + 3);
    } else {
#pragma unroll
      for (int z = 0; z < 4; ++z)
        if (z < len) { key[e + z] = o[z]; pay[e + z] = (int32_t)(e + z); }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_adj_idx(const ull *__restrict__ key, int64_t nnz, int32_t *__restrict__ idx, ull *repeats) {
  ull eq = 0;
  for (int64_t e = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 4; e < nnz; e += (int64_t)gridDim.x * BLOCK * 4) {
    const int len = nnz - e >= 4 ? 4 : (int)(nnz - e);
    ull prev = e > 0 ? key[e - 1] : 0;
    int32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int z = 0; z < 4; ++z)
      if (z < len) {
        const ull k = key[e + z];
        o[z] = (int32_t)(uint32_t)k;
        if (e + z > 0) eq += k == prev;
        prev = k;
      }
    if (len == 4) *reinterpret_cast<int4 *>(idx + e) = make_int4(o[0], o[1], o[2], o[3]);      // (idx: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < 4; ++z)
        if (z < len) idx[e + z] = o[z];
    }
  }
  for (int o = 32; o >= 1; o >>= 1) eq += __shfl_xor(eq, o, 64);
  if ((threadIdx.x & 63) == 0 && eq) atomicAdd(repeats, eq);      // (an integer count: the order of the additions changes nothing)
}

__global__ __launch_bounds__(BLOCK) void k_adj_ptr(const ull *__restrict__ key, int64_t nnz, int64_t n, int32_t *__restrict__ ptr) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i <= n; i += (int64_t)gridDim.x * BLOCK) {
    int64_t lo = 0, hi = nnz;      // first sorted entry whose row is >= i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)(key[mid] >> 32) < i) lo = mid + 1;
      else hi = mid;
    }
    ptr[i] = (int32_t)lo;
  }
}

template <class U, bool CONJ>
__global__ __launch_bounds__(BLOCK) void k_adj_gather(const U *__restrict__ vals, const int32_t *__restrict__ src, int64_t nnz, U *__restrict__ out) {
  constexpr int VPT = 16 / (int)sizeof(U);
  for (int64_t e = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * VPT; e < nnz; e += (int64_t)gridDim.x * BLOCK * VPT) {
    const int len = nnz - e >= VPT ? VPT : (int)(nnz - e);
    Pack16<U> v;
#pragma unroll
    for (int z = 0; z < VPT; ++z)
      if (z < len) v.v[z] = unit_op<CONJ>(vals[src[e + z]]);
    if (len == VPT) *reinterpret_cast<Pack16<U> *>(out + e) = v;      // (out: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)      // (constant indices: the pack stays in registers)
        if (z < len) out[e + z] = v.v[z];
    }
  }
}

template <class U, bool CONJ, int TILE>
__global__ __launch_bounds__(BLOCK) void k_adj_dense(const U *__restrict__ A, int64_t lda, int64_t n, int64_t nt, U *__restrict__ out) {
  constexpr int VPT = 16 / (int)sizeof(U), CH = TILE / VPT, LD = TILE + 1;
  __shared__ U t[TILE * LD];
  const int64_t i0 = ((int64_t)blockIdx.x % nt) * TILE, j0 = ((int64_t)blockIdx.x / nt) * TILE;      // first row / column of the parent's tile
  for (int w = threadIdx.x; w < TILE * CH; w += BLOCK) {      // column by column of the parent, VPT consecutive rows per thread
    const int c = w / CH, r0 = (w - c * CH) * VPT;
    const int64_t i = i0 + r0, j = j0 + c;
    if (i >= n || j >= n) continue;
    const U *from = A + j * lda + i;
    if (i + VPT <= n && (reinterpret_cast<uintptr_t>(from) & 15u) == 0) {
      const Pack16<U> v = *reinterpret_cast<const Pack16<U> *>(from);
#pragma unroll
      for (int z = 0; z < VPT; ++z) t[c * LD + r0 + z] = v.v[z];
    } else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)
        if (i + z < n) t[c * LD + r0 + z] = from[z];
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < TILE * CH; w += BLOCK) {      // column by column of the copy (row r of the parent's tile), VPT consecutive rows
    const int r = w / CH, c0 = (w - r * CH) * VPT;
    const int64_t i = i0 + r, j = j0 + c0;
    if (i >= n || j >= n) continue;
    U *to = out + i * n + j;
    Pack16<U> v;
#pragma unroll
    for (int z = 0; z < VPT; ++z)
      if (j + z < n) v.v[z] = unit_op<CONJ>(t[(c0 + z) * LD + r]);
    if (j + VPT <= n && (reinterpret_cast<uintptr_t>(to) & 15u) == 0) *reinterpret_cast<Pack16<U> *>(to) = v;
    else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)
        if (j + z < n) to[z] = v.v[z];
    }
  }
}

void check_launch(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + hipGetErrorString(e));
}

template <class U, bool CONJ>
void gather_U(hipStream_t s, const void *vals, const int32_t *src, int64_t nnz, void *out) {
  hipLaunchKernelGGL((k_adj_gather<U, CONJ>), dim3(grid_for(nnz, BLOCK * (16 / (int)sizeof(U)))), dim3(BLOCK), 0, s, static_cast<const U *>(vals), src, nnz,
                     static_cast<U *>(out));
}
template <class U, bool CONJ, int TILE>
void dense_U(hipStream_t s, const void *A, int64_t lda, int64_t n, void *out) {
  const int64_t nt = (n + TILE - 1) / TILE;
  if (nt * nt > 0x7fffffffLL) throw std::runtime_error("adj_dense_transpose: n out of range");
  hipLaunchKernelGGL((k_adj_dense<U, CONJ, TILE>), dim3((unsigned)(nt * nt)), dim3(BLOCK), 0, s, static_cast<const U *>(A), lda, n, nt, static_cast<U *>(out));
}
}  // namespace

int adj_dense_tile(int value_bytes) { return value_bytes == 16 ? ADJ_TILE16 : ADJ_TILE; }

void adj_keys(hipStream_t s, const int32_t *rowptr, const int32_t *col, const int32_t *p, int64_t n, int64_t nnz, unsigned long long *key,
              int32_t *pay) {
  if (n < 0 || nnz < 0 || n > 0x7fffffffLL || nnz > 0x7fffffffLL || ((reinterpret_cast<uintptr_t>(key) | reinterpret_cast<uintptr_t>(pay)) & 15u) != 0)
    throw std::runtime_error("adj_keys: bad sizes / output alignment");
  if (nnz == 0) return;
  hipLaunchKernelGGL(k_adj_key, dim3((unsigned)((nnz + ADJ_KEY_TILE - 1) / ADJ_KEY_TILE)), dim3(BLOCK), 0, s, rowptr, col, p, n, nnz, key, pay);
  check_launch("adj_keys");
}

void adj_pattern(hipStream_t s, const unsigned long long *key, int64_t n, int64_t nnz, int32_t *ptr32, int32_t *idx32, unsigned long long *repeats) {
  if (n < 0 || nnz < 0 || n > 0x7fffffffLL || nnz > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(idx32) & 15u) != 0)
    throw std::runtime_error("adj_pattern: bad sizes / output alignment");
  if (hipMemsetAsync(repeats, 0, sizeof(ull), s) != hipSuccess) throw std::runtime_error("adj_pattern: hipMemsetAsync failed");
  if (nnz > 0) hipLaunchKernelGGL(k_adj_idx, dim3(grid_for(nnz, BLOCK * 16)), dim3(BLOCK), 0, s, key, nnz, idx32, repeats);
  hipLaunchKernelGGL(k_adj_ptr, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, s, key, nnz, n, ptr32);
  check_launch("adj_pattern");
}

void adj_gather_values(hipStream_t s, int value_bytes, bool conj, const void *vals, const int32_t *src, int64_t nnz, void *out) {
  if (nnz < 0 || nnz > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(out) & 15u) != 0) throw std::runtime_error("adj_gather_values: bad nnz / output alignment");
  if (conj && value_bytes == 4) throw std::runtime_error("adj_gather_values: 4-byte elements have no conjugate");
  if (nnz == 0) return;
  if (value_bytes == 4) gather_U<uint32_t, false>(s, vals, src, nnz, out);
  else if (value_bytes == 8 && !conj) gather_U<ull, false>(s, vals, src, nnz, out);
  else if (value_bytes == 8) gather_U<ull, true>(s, vals, src, nnz, out);
  else if (value_bytes == 16 && !conj) gather_U<U16, false>(s, vals, src, nnz, out);
  else if (value_bytes == 16) gather_U<U16, true>(s, vals, src, nnz, out);
  else throw std::runtime_error("adj_gather_values: value_bytes must be 4, 8 or 16");
  check_launch("adj_gather_values");
}

void adj_dense_transpose(hipStream_t s, int value_bytes, bool conj, const void *A, int64_t lda, int64_t n, void *out) {
  if (n < 0 || lda < n) throw std::runtime_error("adj_dense_transpose: bad n / lda");
  if (conj && value_bytes == 4) throw std::runtime_error("adj_dense_transpose: 4-byte elements have no conjugate");
  if (n == 0) return;
  if (value_bytes == 4) dense_U<uint32_t, false, ADJ_TILE>(s, A, lda, n, out);
  else if (value_bytes == 8 && !conj) dense_U<ull, false, ADJ_TILE>(s, A, lda, n, out);
  else if (value_bytes == 8) dense_U<ull, true, ADJ_TILE>(s, A, lda, n, out);
  else if (value_bytes == 16 && !conj) dense_U<U16, false, ADJ_TILE16>(s, A, lda, n, out);
  else if (value_bytes == 16) dense_U<U16, true, ADJ_TILE16>(s, A, lda, n, out);
  else throw std::runtime_error("adj_dense_transpose: value_bytes must be 4, 8 or 16");
  check_launch("adj_dense_transpose");
}

}  // namespace dev
}  // namespace expv_mi
