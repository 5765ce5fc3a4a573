// op_bsr.hip -- a caller's block-compressed arrays (BSR / BSC, square blocks), checked and normalised by op_ingest.hip, expanded on
// the device into the scalar CSR32 / CSC32 pattern and value order that create_sparse_device's tail takes
// (capi.hip: expv_mi_op_create_bsr_loc, and expv_mi_op_update_values of an operator born there).
//
// The position contract (include/expv_mi.h).  bd = block_dim, ptr / idx the zero-based block arrays of nb compressed block rows
// (BSR) or block columns (BSC).  Block k = ptr[b] + kk of compressed block b, cnt = ptr[b + 1] - ptr[b], holds the element with
// OUTER in-block index o (BSR: its row r, BSC: its column c) and INNER in-block index i (BSR: c, BSC: r) at scalar position
//     p = bd^2 ptr[b] + o bd cnt + kk bd + i,     scalar index  idx[k] bd + i,     scalar ptr[b bd + o] = bd^2 ptr[b] + o bd cnt
// -- scipy's bsr_matrix((vals, idx, ptr)).tocsr(), stored zeros and the caller's block order inside a block row kept.  In the
// caller's values that element lies at k bd^2 + o bd + i when the blocks are stored outer-major (BSR row-major, BSC column-major)
// and at k bd^2 + i bd + o otherwise ("transposed").
//
// All three kernels are OUTPUT-parallel: a thread owns consecutive scalar positions, finds where they come from and writes them
// with one 16-byte store, so the writes of a wave are contiguous whatever bd is; nothing assumes that a block fits a wave or a
// workgroup.
//   k_bsr_ptr      one thread per scalar row (column) j <= n: ptr32[j] from the formula above, ptr32[n] = nnz.
//   k_bsr_idx      BSR_TILE positions per workgroup, four per thread and trip: idx32[p] = idx[k] bd + i.
//   k_bsr_vals     BSR_TILE positions per workgroup, 16 bytes per thread and trip: out[p] = vals[source of p].  Used at creation and
//                  by every value refresh.  Elements move as raw 4- / 8- / 16-byte units (a permutation: no arithmetic, no
//                  atomics), so the four element types share three instantiations.  A caller's array aligned to 16 bytes whose
//                  blocks are outer-major with bd a multiple of the units per 16 bytes is read with 16-byte loads (every group of
//                  positions a thread owns is then contiguous and aligned in the source); anything else by single units.
// Where position p comes from: its compressed block b is the one with ptr[b] <= p / bd^2 < ptr[b + 1] -- a bisection, run once
// by the workgroup for the two ends of its tile and then per thread inside that range (a few steps: a tile covers few block rows
// unless they are empty); o, kk, i are two 32-bit divisions of p - bd^2 ptr[b] (< 2^31: the scalar pattern is CSR32).  The
// following positions of the thread are reached by stepping (i, kk, o, b), empty block rows skipped.  Positions are formed in 64-bit
// arithmetic before they are narrowed.
//
// Unchecked values: none.  Every launch here is issued behind the status read-back of ingest_indices on the block arrays, i.e.
// for ptr[0] = 0 <= ... non-decreasing ... <= ptr[nb] = nnzb and idx in [0, nb).
// Memory: no LDS, no scratch, no temporaries.  Traffic of k_bsr_vals: one read and one write of every value.
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"

namespace expv_mi {
namespace dev {

namespace {
typedef unsigned long long ull;
constexpr int BSR_TILE = 9216;                      // scalar positions a workgroup expands (idx and vals): 36 BLOCK = 9 * 1024
static_assert(BSR_TILE % (BLOCK * 4) == 0, "whole trips of four positions per thread");

struct U16 { ull a, b; };                           // a 16-byte element, 8-byte aligned in a caller's array
template <class U> struct alignas(16) Pack16 { U v[16 / sizeof(U)]; };

// where a scalar position comes from
struct Cursor {
  int32_t b, first;        // compressed block row (column), ptr[b]
  uint32_t cnt, o, kk, i;  // blocks in it; outer in-block index, block inside the row, inner in-block index
};
// the b in [lo, hi] with ptr[b] <= kb < ptr[b + 1]; the caller knows that there is one
__device__ __forceinline__ int32_t find_block_row(const int32_t *__restrict__ ptr, int32_t lo, int32_t hi, int32_t kb) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid + 1] > kb) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ Cursor locate(const int32_t *__restrict__ ptr, uint32_t bd, uint32_t bd2, int64_t p, int32_t lo, int32_t hi) {
  Cursor c;
  c.b = find_block_row(ptr, lo, hi, (int32_t)((uint32_t)p / bd2));
  c.first = ptr[c.b];
  c.cnt = (uint32_t)(ptr[c.b + 1] - c.first);
  const uint32_t q = (uint32_t)(p - (int64_t)bd2 * c.first), w = bd * c.cnt;
  c.o = q / w;
  const uint32_t rem = q - c.o * w;
  c.kk = rem / bd;
  c.i = rem - c.kk * bd;
  return c;
}
// the next position (the caller knows that there is one)
__device__ __forceinline__ void advance(Cursor &c, const int32_t *__restrict__ ptr, uint32_t bd, int32_t nb) {
  if (++c.i < bd) return;
  c.i = 0;
  if (++c.kk < c.cnt) return;
  c.kk = 0;
  if (++c.o < bd) return;
  c.o = 0;
  int32_t b = c.b + 1, a = ptr[b], e = a;
  while (b < nb && (e = ptr[b + 1]) == a) ++b;      // (empty block rows)
  c.b = b;
  c.first = a;
  c.cnt = (uint32_t)(e - a);
}
// the block rows a workgroup's tile [p0, p1] lies in
struct Range { int32_t lo, hi; };
__device__ __forceinline__ Range tile_range(const int32_t *__restrict__ ptr, int32_t nb, uint32_t bd2, int64_t p0, int64_t p1) {
  Range r;
  r.lo = find_block_row(ptr, 0, nb - 1, (int32_t)((uint32_t)p0 / bd2));
  r.hi = find_block_row(ptr, r.lo, nb - 1, (int32_t)((uint32_t)p1 / bd2));
  return r;
}

__global__ __launch_bounds__(BLOCK) void k_bsr_ptr(const int32_t *__restrict__ ptr, int64_t n, int64_t nnz, uint32_t bd, int32_t *__restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j <= n; j += (int64_t)gridDim.x * BLOCK) {
    int64_t v = nnz;
    if (j < n) {
      const uint32_t b = (uint32_t)j / bd, o = (uint32_t)j - b * bd;
      const int64_t first = ptr[b], cnt = ptr[b + 1] - first;
      v = (int64_t)bd * bd * first + (int64_t)o * bd * cnt;
    }
    out[j] = (int32_t)v;
  }
}

__global__ __launch_bounds__(BLOCK) void k_bsr_idx(const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx, int32_t nb, int64_t nnz,
                                                   uint32_t bd, int32_t *__restrict__ out) {
  const uint32_t bd2 = bd * bd;
  const int64_t p0 = (int64_t)blockIdx.x * BSR_TILE, pend = p0 + BSR_TILE < nnz ? p0 + BSR_TILE : nnz;
  const Range rg = tile_range(ptr, nb, bd2, p0, pend - 1);
  for (int64_t p = p0 + (int64_t)threadIdx.x * 4; p < pend; p += BLOCK * 4) {
    const int len = pend - p >= 4 ? 4 : (int)(pend - p);
    Cursor c = locate(ptr, bd, bd2, p, rg.lo, rg.hi);
    int32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int z = 0; z < 4; ++z)
      if (z < len) {
        if (z) advance(c, ptr, bd, nb);
        o[z] = (int32_t)((int64_t)idx[c.first + (int32_t)c.kk] * bd + c.i);
      }
    if (len == 4) *reinterpret_cast<int4 *>(out + p) = make_int4(o[0], o[1], o[2], o[3]);      // (out: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < 4; ++z)
        if (z < len) out[p + z] = o[z];
    }
  }
}

template <class U, bool WIDE>
__global__ __launch_bounds__(BLOCK) void k_bsr_vals(const int32_t *__restrict__ ptr, const U *__restrict__ vals, int32_t nb, int64_t nnz, uint32_t bd,
                                                    bool transposed, U *__restrict__ out) {
  constexpr int VPT = 16 / (int)sizeof(U);
  const uint32_t bd2 = bd * bd;
  const int64_t p0 = (int64_t)blockIdx.x * BSR_TILE, pend = p0 + BSR_TILE < nnz ? p0 + BSR_TILE : nnz;
  const Range rg = tile_range(ptr, nb, bd2, p0, pend - 1);
  for (int64_t p = p0 + (int64_t)threadIdx.x * VPT; p < pend; p += BLOCK * VPT) {
    const int len = pend - p >= VPT ? VPT : (int)(pend - p);
    Cursor c = locate(ptr, bd, bd2, p, rg.lo, rg.hi);
    Pack16<U> v;
    if (WIDE) {      // outer-major blocks, bd a multiple of VPT (so len == VPT), vals on 16 bytes: the thread's positions are one aligned pack
      v = *reinterpret_cast<const Pack16<U> *>(vals + ((int64_t)(c.first + (int32_t)c.kk) * bd2 + c.o * bd + c.i));
    } else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)
        if (z < len) {
          if (z) advance(c, ptr, bd, nb);
          v.v[z] = vals[(int64_t)(c.first + (int32_t)c.kk) * bd2 + (transposed ? c.i * bd + c.o : c.o * bd + c.i)];
        }
    }
    if (len == VPT) *reinterpret_cast<Pack16<U> *>(out + p) = v;      // (out: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)      // (constant indices: the pack stays in registers)
        if (z < len) out[p + z] = v.v[z];
    }
  }
}

void check_launch(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + hipGetErrorString(e));
}

template <class U>
void permute_U(hipStream_t s, const int32_t *ptr, const void *vals, int32_t nb, int64_t nnz, uint32_t bd, bool transposed, void *out) {
  constexpr int VPT = 16 / (int)sizeof(U);
  const dim3 g((unsigned)((nnz + BSR_TILE - 1) / BSR_TILE));
  const bool wide = !transposed && bd % VPT == 0 && (reinterpret_cast<uintptr_t>(vals) & 15u) == 0;
  if (wide)
    hipLaunchKernelGGL((k_bsr_vals<U, true>), g, dim3(BLOCK), 0, s, ptr, static_cast<const U *>(vals), nb, nnz, bd, transposed, static_cast<U *>(out));
  else
    hipLaunchKernelGGL((k_bsr_vals<U, false>), g, dim3(BLOCK), 0, s, ptr, static_cast<const U *>(vals), nb, nnz, bd, transposed, static_cast<U *>(out));
}
}  // namespace

int bsr_tile() { return BSR_TILE; }

void bsr_expand_pattern(hipStream_t s, const int32_t *bptr, const int32_t *bidx, int64_t nb, int64_t nnzb, int block_dim, int32_t *ptr32,
                        int32_t *idx32) {
  const int64_t n = nb * block_dim, nnz = nnzb * block_dim * block_dim;
  if (block_dim < 1 || nb < 0 || nnzb < 0 || n > 0x7fffffffLL || nnz > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(idx32) & 15u) != 0)
    throw std::runtime_error("bsr_expand_pattern: bad sizes / output alignment");
  hipLaunchKernelGGL(k_bsr_ptr, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, s, bptr, n, nnz, (uint32_t)block_dim, ptr32);
  if (nnz > 0)
    hipLaunchKernelGGL(k_bsr_idx, dim3((unsigned)((nnz + BSR_TILE - 1) / BSR_TILE)), dim3(BLOCK), 0, s, bptr, bidx, (int32_t)nb, nnz,
                       (uint32_t)block_dim, idx32);
  check_launch("bsr_expand_pattern");
}

void bsr_permute_values(hipStream_t s, int value_bytes, const int32_t *bptr, const void *vals, int64_t nb, int64_t nnzb, int block_dim,
                        bool transposed, void *out) {
  const int64_t nnz = nnzb * block_dim * block_dim;
  if (block_dim < 1 || nb < 0 || nnzb < 0 || nnz > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
    throw std::runtime_error("bsr_permute_values: bad sizes / output alignment");
  if (nnz == 0) return;
  if (value_bytes == 4) permute_U<uint32_t>(s, bptr, vals, (int32_t)nb, nnz, (uint32_t)block_dim, transposed, out);
  else if (value_bytes == 8) permute_U<ull>(s, bptr, vals, (int32_t)nb, nnz, (uint32_t)block_dim, transposed, out);
  else if (value_bytes == 16) permute_U<U16>(s, bptr, vals, (int32_t)nb, nnz, (uint32_t)block_dim, transposed, out);
  else throw std::runtime_error("bsr_permute_values: value_bytes must be 4, 8 or 16");
  check_launch("bsr_permute_values");
}

}  // namespace dev
}  // namespace expv_mi
