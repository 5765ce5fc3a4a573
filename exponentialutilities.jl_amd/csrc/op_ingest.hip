// op_ingest.hip -- a caller's CSR / CSC index arrays, resident on the device, checked and normalised there
// (capi.hip: expv_mi_op_create_csr_loc / _csc_loc with loc = EXPV_MI_DEVICE).
//
// The arrays come from somebody else's code (torch, rocSPARSE, a ROCSparseMatrixCSR): 4- or 8-byte integers, index base 0 or 1,
// and nothing about them is known to hold.  Two streaming kernels turn them into the library's own zero-based CSR32 / CSC32 copies
// and fill one status record that the host reads back once; neither kernel indexes memory by a value it has read -- the one
// exception, the look at the first entry of every row, is guarded by the caller's own buffer length.  Everything that does index by
// these arrays (the host planners, the fill of the stored forms) runs after the host has seen a clean status.
//
//   k_ingest_ptr   rowptr (colptr): ptr[0] == base, non-decreasing, ptr[n] - base == the nnz the caller states; int32 copy.
//                  Also counts the rows whose FIRST entry does not exceed the entry stored before it (see below).
//   k_ingest_idx   colind (rowval): every index in [0, n) after the base is taken off; int32 copy; counts the entries k >= 1
//                  with idx[k] <= idx[k - 1].  16-byte loads and stores, four entries per lane and trip.
//
// Rows sorted and free of duplicates (the condition of the device Hermitian test: kernels.hip, k_op_update_forms) means: no entry
// inside a row is <= its predecessor.  Entry-parallel, that is the count of ALL k with idx[k] <= idx[k - 1] minus those k that
// start a row (where the predecessor belongs to another row): desc_all == desc_starts.  No thread walks a row.
//
// Traffic: nnz idx_bytes + (n + 1) idx_bytes in, 4 (nnz + n + 1) out, once per creation.  Flags and counts are reduced per
// workgroup (wave shuffles, then LDS) and leave it with at most one atomic per status word; a clean, sorted input issues none.
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"

namespace expv_mi {
namespace dev {

namespace {
typedef unsigned long long ull;
constexpr ull NOPOS = ~0ull;

__device__ __forceinline__ ull wave_or(ull v) {
  for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ ull wave_min(ull v) {
  for (int o = 32; o >= 1; o >>= 1) { const ull w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ ull wave_add(ull v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// flags / first offending position / a count of one workgroup -> the status record (thread 0, only what is not neutral)
__device__ __forceinline__ void publish(ull flags, ull pos, ull cnt, ull *st_flags, ull *st_pos, ull *st_cnt) {
  __shared__ ull sh[3][BLOCK / 64];
  flags = wave_or(flags);
  pos = wave_min(pos);
  cnt = wave_add(cnt);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][w] = flags; sh[1][w] = pos; sh[2][w] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < BLOCK / 64; ++q) {
      flags |= sh[0][q];
      pos = sh[1][q] < pos ? sh[1][q] : pos;
      cnt += sh[2][q];
    }
    if (flags) atomicOr(st_flags, flags);
    if (pos != NOPOS) atomicMin(st_pos, pos);
    if (cnt) atomicAdd(st_cnt, cnt);
  }
}

template <class I>
__global__ __launch_bounds__(BLOCK) void k_ingest_ptr(const I *__restrict__ ptr, const I *__restrict__ idx, int64_t n, int64_t nnz,
                                                      int64_t base, int32_t *__restrict__ ptr32, IngestStatus *st) {
  ull flags = 0, pos = NOPOS, starts = 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i <= n; i += (int64_t)gridDim.x * BLOCK) {
    const int64_t a = (int64_t)ptr[i] - base;
    if (i == 0 && a != 0) { flags |= INGEST_BAD_FIRST; pos = 0; }
    if (i < n) {
      const int64_t b = (int64_t)ptr[i + 1] - base;
      if (b < a) { flags |= INGEST_DECREASING; pos = pos < (ull)(i + 1) ? pos : (ull)(i + 1); }
      // a non-empty row whose first entry has a predecessor: inside the caller's nnz entries whatever ptr claims
      if (b > a && a >= 1 && a < nnz && idx[a] <= idx[a - 1]) ++starts;
    } else if (a != nnz) {
      flags |= INGEST_BAD_NNZ;
      pos = pos < (ull)n ? pos : (ull)n;
    }
    ptr32[i] = (int32_t)a;      // (of a refused input: never read)
  }
  publish(flags, pos, starts, &st->flags, &st->first_ptr, &st->desc_starts);
}

template <class I> struct Quad { I v[4]; };
template <class I, bool VEC>
__device__ __forceinline__ Quad<I> load4(const I *p) {
  Quad<I> q;
  if (VEC) {      // 16-byte loads: one for four 4-byte indices, two for four 8-byte ones
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
    uint4 w[sizeof(I) / 4];
#pragma unroll
    for (int z = 0; z < (int)(sizeof(I) / 4); ++z) w[z] = p4[z];
    __builtin_memcpy(&q, w, sizeof(q));
  } else {
#pragma unroll
    for (int z = 0; z < 4; ++z) q.v[z] = p[z];
  }
  return q;
}
template <class I, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_ingest_idx(const I *__restrict__ idx, int64_t n, int64_t nnz, int64_t base,
                                                      int32_t *__restrict__ idx32, IngestStatus *st) {
  ull flags = 0, pos = NOPOS, desc = 0;
  for (int64_t k = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 4; k < nnz; k += (int64_t)gridDim.x * BLOCK * 4) {
    Quad<I> q;
    const int len = nnz - k >= 4 ? 4 : (int)(nnz - k);
    if (len == 4) q = load4<I, VEC>(idx + k);
    else
      for (int z = 0; z < 4; ++z) q.v[z] = z < len ? idx[k + z] : (I)base;
    I prev = k > 0 ? idx[k - 1] : q.v[0];      // (the neighbouring lane's last entry: a cache hit)
    int32_t o[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) {
      const int64_t c = (int64_t)q.v[z] - base;
      if (z < len) {
        if (c < 0 || c >= n) { flags |= INGEST_BAD_INDEX; pos = pos < (ull)(k + z) ? pos : (ull)(k + z); }
        if ((k + z) > 0 && q.v[z] <= prev) ++desc;
        prev = q.v[z];
      }
      o[z] = (int32_t)c;
    }
    if (len == 4) *reinterpret_cast<int4 *>(idx32 + k) = make_int4(o[0], o[1], o[2], o[3]);      // (idx32: the library's buffer, 16-byte aligned)
    else
      for (int z = 0; z < len; ++z) idx32[k + z] = o[z];
  }
  publish(flags, pos, desc, &st->flags, &st->first_idx, &st->desc_all);
}

template <class I>
void ingest_T(hipStream_t s, const void *ptr, const void *idx, int64_t n, int64_t nnz, int base, int32_t *ptr32, int32_t *idx32,
              IngestStatus *st) {
  const I *p = static_cast<const I *>(ptr), *x = static_cast<const I *>(idx);
  hipLaunchKernelGGL(k_ingest_ptr<I>, dim3(grid_for(n + 1, BLOCK * 4)), dim3(BLOCK), 0, s, p, x, n, nnz, (int64_t)base, ptr32, st);
  if (nnz > 0) {
    const dim3 g(grid_for(nnz, BLOCK * 16));
    if ((reinterpret_cast<uintptr_t>(idx) & 15u) == 0)
      hipLaunchKernelGGL((k_ingest_idx<I, true>), g, dim3(BLOCK), 0, s, x, n, nnz, (int64_t)base, idx32, st);
    else      // (a view into somebody's storage need not start on 16 bytes)
      hipLaunchKernelGGL((k_ingest_idx<I, false>), g, dim3(BLOCK), 0, s, x, n, nnz, (int64_t)base, idx32, st);
  }
}
}  // namespace

void ingest_indices(hipStream_t s, int idx_bytes, const void *ptr, const void *idx, int64_t n, int64_t nnz, int base, int32_t *ptr32,
                    int32_t *idx32, IngestStatus *st) {
  if (idx_bytes != 4 && idx_bytes != 8) throw std::runtime_error("ingest_indices: idx_bytes must be 4 or 8");
  if (n < 0 || nnz < 0 || (reinterpret_cast<uintptr_t>(idx32) & 15u) != 0) throw std::runtime_error("ingest_indices: bad n / nnz / output alignment");
  // the record: flags and counts 0, first offending positions "none"
  if (hipMemsetAsync(st, 0, sizeof(IngestStatus), s) != hipSuccess || hipMemsetAsync(&st->first_ptr, 0xff, 2 * sizeof(ull), s) != hipSuccess)
    throw std::runtime_error("ingest_indices: hipMemsetAsync failed");
  if (idx_bytes == 8) ingest_T<int64_t>(s, ptr, idx, n, nnz, base, ptr32, idx32, st);
  else ingest_T<int32_t>(s, ptr, idx, n, nnz, base, ptr32, idx32, st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string("ingest_indices: ") + hipGetErrorString(e));
}

}  // namespace dev
}  // namespace expv_mi
