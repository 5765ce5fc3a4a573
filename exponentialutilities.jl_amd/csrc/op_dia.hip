// op_dia.hip -- a caller's stored diagonals (DIA / banded: ndiag rows of ld elements and ndiag offsets), checked on the host by
// capi.hip: validate_dia, expanded on the device into the scalar CSR32 pattern and value order that finish_sparse_device's tail
// takes (capi.hip: expv_mi_op_create_dia_loc, and expv_mi_op_update_values of an operator born there).
//
// The position contract (include/expv_mi.h).  off[0] < ... < off[q - 1] are the caller's offsets with |k| < n in ascending order
// and base[r] the element index into `data` of row 0 of diagonal r: element (i, i + off[r]) lies at data[base[r] + i] under all
// three alignments (base[r] = d(r) ld + off[r] for COL, d(r) ld for ROW, d(r) ld + min(0, off[r]) for START; d(r) the caller's row of
// `data`).  Row i stores the diagonals r with 0 <= i + off[r] < n -- a contiguous range [lo_i, lo_i + cnt_i) of r, lo_i the first r
// with off[r] >= -i -- in ascending r at positions rowptr[i] + (r - lo_i), column i + off[r], and
//     rowptr[i] = sum_r clamp(min(i, n - off[r]) - max(0, -off[r]), 0, n - |off[r]|)        (dia_rowptr, in 64-bit arithmetic)
// which is scipy's dia_matrix((data, offsets)).tocsr() with stored zeros kept.  The pattern depends on the offsets alone.
//
// Ownership.  Every kernel is parallel over what it WRITES and nothing is written twice: no atomics, no temporaries.
//   k_dia_ptr    one thread per scalar row j <= n: ptr32[j] from the closed form, ptr32[n] = nnz.
//   k_dia_idx    DIA_POS_TILE positions per workgroup, four per thread and trip, one 16-byte store: the row of a position by
//                bisection on ptr32 (first for the two ends of the tile, then per thread inside that range), its diagonal
//                lo_i + (p - ptr32[i]), the following positions by stepping (diagonal, then row; empty rows skipped).
//   k_dia_vals   the transposition; creation and every value refresh.  A workgroup owns `rows` consecutive rows (DIA_TILE, halved
//                while (q | 1) rows value_bytes exceeds DIA_LDS_BYTES, which happens beyond q = DIA_Q_FULL diagonals) and with
//                them the contiguous output range [rowptr[r0], rowptr[r0 + rows)).  It forms its rowptr values by the closed form
//                in LDS (so a refresh needs nothing but the offsets table), then
//                  STAGED (q <= DIA_Q_LDS): reads every diagonal's segment for its rows with contiguous loads -- 16 bytes wide
//                    where the group of rows lies inside the diagonal's in-matrix extent and its address is 16-byte aligned,
//                    single elements otherwise -- into the LDS image sv[t (q | 1) + (r - lo_t)], t the row inside the tile: the row
//                    stride is ODD, so the stores of consecutive rows of one diagonal fall into different banks for 4-, 8- and
//                    16-byte elements alike (two rows per lane at 8 bytes, four at 4 bytes: a 2- / 4-way conflict on the store
//                    only); then writes the output range from LDS with 16-byte stores, packs aligned in the OUTPUT buffer (the first
//                    and last pack of a workgroup's range may be partial and are written element by element).
//                  GATHER (q > DIA_Q_LDS): the same output loop reads data[base[r] + i] directly.
//                Values move as raw 4- / 8- / 16-byte units (a permutation: no arithmetic), so the four element types share three
//                instantiations.  Nothing assumes that q fits a wave, that a row has all q entries, or anything about ld.
//
// Padding is never read: a value is loaded only for a pair (i, r) with 0 <= i + off[r] < n, and the wide load only when all its
// rows satisfy that.  Unchecked values: none are indexed by -- off / base come from the host's validate_dia (|off[r]| < n, strictly
// ascending, base[r] + i inside the caller's ndiag x ld array for every in-matrix i), and every launch is issued after it passed.
// Memory: (q | 1) rows value_bytes + 4 (2 rows + 1) bytes of dynamic LDS per workgroup, at most DIA_LDS_BYTES + 8 (DIA_TILE + 1) (about
// 38 KiB: four workgroups per CU; the five Float64 diagonals of the headline operator take 12 KiB: eight), no scratch.
// Traffic of k_dia_vals: one read and one write of every value.
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"

namespace expv_mi {
namespace dev {

namespace {
typedef unsigned long long ull;
constexpr int DIA_TILE = 256;                       // rows a workgroup of k_dia_vals owns (one per thread while sizes are formed)
constexpr int DIA_TILE_MIN = 32;                    // ... and the fewest it is shrunk to
constexpr int DIA_Q_FULL = 8;                       // in-range diagonals up to which every element type keeps the whole tile
constexpr int DIA_Q_LDS = 64;                       // in-range diagonals beyond which the values are gathered directly, not staged
constexpr int DIA_LDS_BYTES = (DIA_Q_FULL + 1) * DIA_TILE * 16;      // the staged values: 36 KiB
constexpr int DIA_POS_TILE = 4096;                  // scalar positions a workgroup of k_dia_idx expands
static_assert(DIA_TILE == BLOCK, "one thread per row of the tile");
static_assert(((DIA_Q_LDS | 1) * DIA_TILE_MIN * 16) <= DIA_LDS_BYTES, "the smallest tile of the widest staged band fits");
static_assert(DIA_LDS_BYTES + 8 * (DIA_TILE + 1) <= 64 * 1024, "LDS of a workgroup");
static_assert(DIA_POS_TILE % (BLOCK * 4) == 0, "whole trips of four positions per thread");

typedef ull U16 __attribute__((ext_vector_type(2), aligned(8)));      // a 16-byte element, 8-byte aligned in a caller's array (a vector type: a struct went through scratch)
template <class U> struct alignas(16) Pack16 { U v[16 / sizeof(U)]; };

// rowptr[i], 0 <= i <= n: the entries of the rows before i, diagonal by diagonal
__device__ __forceinline__ int64_t dia_rowptr(const int32_t *__restrict__ off, int q, int64_t n, int64_t i) {
  int64_t sum = 0;
  for (int r = 0; r < q; ++r) {
    const int64_t s = off[r], first = s < 0 ? -s : 0, len = n - (s < 0 ? -s : s);
    int64_t c = (i < n - s ? i : n - s) - first;
    c = c < 0 ? 0 : (c > len ? len : c);
    sum += c;
  }
  return sum;
}
// lo_i: the first r with off[r] >= -i (q when there is none)
__device__ __forceinline__ int first_diag(const int32_t *__restrict__ off, int q, int64_t i) {
  int lo = 0, hi = q;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)off[mid] < -i) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// the i in [lo, hi] with ptr[i] <= p < ptr[i + 1]; the caller knows that there is one
__device__ __forceinline__ int64_t find_row(const int32_t *__restrict__ ptr, int64_t lo, int64_t hi, int32_t p) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid + 1] > p) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(BLOCK) void k_dia_ptr(const int32_t *__restrict__ off, int q, int64_t n, int64_t nnz, int32_t *__restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j <= n; j += (int64_t)gridDim.x * BLOCK)
    out[j] = (int32_t)(j < n ? dia_rowptr(off, q, n, j) : nnz);
}

__global__ __launch_bounds__(BLOCK) void k_dia_idx(const int32_t *__restrict__ ptr, const int32_t *__restrict__ off, int q, int64_t n, int64_t nnz,
                                                   int32_t *__restrict__ out) {
  const int64_t p0 = (int64_t)blockIdx.x * DIA_POS_TILE, pend = p0 + DIA_POS_TILE < nnz ? p0 + DIA_POS_TILE : nnz;
  const int64_t rlo = find_row(ptr, 0, n - 1, (int32_t)p0), rhi = find_row(ptr, rlo, n - 1, (int32_t)(pend - 1));
  for (int64_t p = p0 + (int64_t)threadIdx.x * 4; p < pend; p += BLOCK * 4) {
    const int len = pend - p >= 4 ? 4 : (int)(pend - p);
    int64_t i = find_row(ptr, rlo, rhi, (int32_t)p);
    int32_t first = ptr[i], cnt = ptr[i + 1] - first, j = (int32_t)p - first;
    int lo = first_diag(off, q, i);
    int32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int z = 0; z < 4; ++z)
      if (z < len) {
        if (j == cnt) {      // the next row that stores anything (there is one: p + z < nnz)
          do { ++i; first += cnt; cnt = ptr[i + 1] - first; } while (cnt == 0);
          j = 0;
          lo = first_diag(off, q, i);
        }
        o[z] = (int32_t)(i + off[lo + j]);
        ++j;
      }
    if (len == 4) *reinterpret_cast<int4 *>(out + p) = make_int4(o[0], o[1], o[2], o[3]);      // (out: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < 4; ++z)
        if (z < len) out[p + z] = o[z];
    }
  }
}

template <class U, bool STAGED>
__global__ __launch_bounds__(BLOCK) void k_dia_vals(const U *__restrict__ data, const int64_t *__restrict__ base, const int32_t *__restrict__ off,
                                                    int q, int64_t n, int rows, U *__restrict__ out) {
  constexpr int VPT = 16 / (int)sizeof(U);
  // dynamic LDS, sized by the launch to what the tile needs (dia_lds_bytes): the staged values first -- (q | 1) rows elements, a
  // multiple of 16 bytes because rows is a multiple of DIA_TILE_MIN --, then rowptr (rows + 1) and lo_i (rows) of the tile's rows
  extern __shared__ __attribute__((aligned(16))) unsigned char dia_lds[];
  const int qs = q | 1;
  U *sv = reinterpret_cast<U *>(dia_lds);
  int32_t *sp = reinterpret_cast<int32_t *>(dia_lds + (STAGED ? (size_t)qs * rows * sizeof(U) : 0));
  int32_t *slo = sp + (rows + 1);
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int nr = n - r0 < rows ? (int)(n - r0) : rows;
  if (tid < nr) {
    sp[tid] = (int32_t)dia_rowptr(off, q, n, r0 + tid);
    slo[tid] = first_diag(off, q, r0 + tid);
  }
  if (tid == BLOCK - 1) sp[nr] = (int32_t)dia_rowptr(off, q, n, r0 + nr);      // (nr may equal BLOCK: one entry more than there are threads)
  __syncthreads();
  if (STAGED) {      // diagonal by diagonal, VPT consecutive rows per thread: contiguous in the caller's array
    const int chunks = rows / VPT;      // (rows and VPT are powers of two)
    for (int w = tid; w < q * chunks; w += BLOCK) {
      const int r = w / chunks, t0 = (w - r * chunks) * VPT;
      if (t0 >= nr) continue;
      const int64_t s = off[r], i0 = r0 + t0, ilo = s < 0 ? -s : 0, ihi = s < 0 ? n : n - s;      // rows [ilo, ihi) hold diagonal r
      const int64_t src = base[r] + i0;
      bool wide = false;
      if (VPT > 1) wide = i0 >= ilo && i0 + VPT <= ihi && (reinterpret_cast<uintptr_t>(data + src) & 15u) == 0;
      if (wide) {
        const Pack16<U> v = *reinterpret_cast<const Pack16<U> *>(data + src);
#pragma unroll
        for (int z = 0; z < VPT; ++z) sv[(t0 + z) * qs + (r - slo[t0 + z])] = v.v[z];
      } else {
#pragma unroll
        for (int z = 0; z < VPT; ++z)
          if (i0 + z >= ilo && i0 + z < ihi) sv[(t0 + z) * qs + (r - slo[t0 + z])] = data[src + z];
      }
    }
    __syncthreads();
  }
  const int32_t pbase = sp[0], pend = sp[nr];
  const bool uniform = (int64_t)(pend - pbase) == (int64_t)nr * q;      // every row of the tile stores all q diagonals
  for (int64_t P = (int64_t)(pbase - pbase % VPT) + (int64_t)tid * VPT; P < pend; P += BLOCK * VPT) {
    const int32_t first = P < pbase ? pbase : (int32_t)P, last = P + VPT < pend ? (int32_t)(P + VPT) : pend;      // [first, last)
    int t, j;
    if (uniform) {
      t = (int)((uint32_t)(first - pbase) / (uint32_t)q);
      j = (first - pbase) - t * q;
    } else {
      int lo = 0, hi = nr - 1;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sp[mid + 1] > first) hi = mid;
        else lo = mid + 1;
      }
      t = lo;
      j = first - sp[t];
    }
    Pack16<U> v;
#pragma unroll
    for (int z = 0; z < VPT; ++z)
      if (P + z >= first && P + z < last) {
        while (j >= sp[t + 1] - sp[t]) { ++t; j = 0; }      // (a later row stores something: P + z < pend)
        if (STAGED) v.v[z] = sv[t * qs + j];
        else v.v[z] = data[base[slo[t] + j] + (r0 + t)];
        ++j;
      }
    if (last - first == VPT) *reinterpret_cast<Pack16<U> *>(out + P) = v;      // (out: the library's buffer, 16-byte aligned)
    else {
#pragma unroll
      for (int z = 0; z < VPT; ++z)      // (constant indices: the pack stays in registers)
        if (P + z >= first && P + z < last) out[P + z] = v.v[z];
    }
  }
}

void check_launch(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + hipGetErrorString(e));
}

template <class U>
void permute_U(hipStream_t s, const void *data, const int64_t *base, const int32_t *off, int q, int64_t n, void *out) {
  const int rows = dia_rows(q, (int)sizeof(U));
  const dim3 g((unsigned)((n + rows - 1) / rows));
  const size_t index_bytes = sizeof(int32_t) * (size_t)(2 * rows + 1);
  if (q <= DIA_Q_LDS)
    hipLaunchKernelGGL((k_dia_vals<U, true>), g, dim3(BLOCK), (size_t)(q | 1) * rows * sizeof(U) + index_bytes, s, static_cast<const U *>(data), base, off, q, n, rows, static_cast<U *>(out));
  else
    hipLaunchKernelGGL((k_dia_vals<U, false>), g, dim3(BLOCK), index_bytes, s, static_cast<const U *>(data), base, off, q, n, rows, static_cast<U *>(out));
}
}  // namespace

int dia_tile() { return DIA_TILE; }
int dia_q_lds() { return DIA_Q_LDS; }
int dia_rows(int q, int value_bytes) {
  int rows = DIA_TILE;
  if (q <= DIA_Q_LDS)
    while (rows > DIA_TILE_MIN && (int64_t)(q | 1) * rows * value_bytes > DIA_LDS_BYTES) rows >>= 1;
  return rows;
}

void dia_expand_pattern(hipStream_t s, const int32_t *off, int q, int64_t n, int64_t nnz, int32_t *ptr32, int32_t *idx32) {
  if (q < 0 || n < 0 || nnz < 0 || n > 0x7fffffffLL || nnz > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(idx32) & 15u) != 0)
    throw std::runtime_error("dia_expand_pattern: bad sizes / output alignment");
  hipLaunchKernelGGL(k_dia_ptr, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, s, off, q, n, nnz, ptr32);
  if (nnz > 0)
    hipLaunchKernelGGL(k_dia_idx, dim3((unsigned)((nnz + DIA_POS_TILE - 1) / DIA_POS_TILE)), dim3(BLOCK), 0, s, ptr32, off, q, n, nnz, idx32);
  check_launch("dia_expand_pattern");
}

void dia_permute_values(hipStream_t s, int value_bytes, const void *data, const int64_t *base, const int32_t *off, int q, int64_t n,
                        int64_t nnz, void *out) {
  if (q < 0 || n < 0 || nnz < 0 || n > 0x7fffffffLL || nnz > 0x7fffffffLL || (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
    throw std::runtime_error("dia_permute_values: bad sizes / output alignment");
  if (nnz == 0) return;
  if (value_bytes == 4) permute_U<uint32_t>(s, data, base, off, q, n, out);
  else if (value_bytes == 8) permute_U<ull>(s, data, base, off, q, n, out);
  else if (value_bytes == 16) permute_U<U16>(s, data, base, off, q, n, out);
  else throw std::runtime_error("dia_permute_values: value_bytes must be 4, 8 or 16");
  check_launch("dia_permute_values");
}

}  // namespace dev
}  // namespace expv_mi
