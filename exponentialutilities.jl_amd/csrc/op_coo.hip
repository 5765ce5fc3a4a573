// op_coo.hip -- a caller's coordinate triplets (row, col, value), resident on the device, sorted, coalesced and compressed there
// into the checked CSR32 pattern that create_sparse_device's tail takes (capi.hip: expv_mi_op_create_coo_loc).
//
// The triplets come in any order and may repeat a coordinate; the stored entry is the sum of the values of its coordinate, taken
// in the operator's element type in ASCENDING ORDER OF THE ENTRY'S POSITION in the caller's arrays (complex: real and imaginary
// parts separately).  That order is the contract (include/expv_mi.h); a stable sort and a left-to-right segment sum keep it, and
// no floating-point atomic appears anywhere, so a creation is reproducible bit for bit.
//
//   1. k_coo_key      one streaming pass over row / col (16-byte loads where the address allows): range check of both indices
//                     (flag + first offending position of each array, as op_ingest.hip publishes them), the zero-based 64-bit
//                     key row << 32 | col, and two counts over the positions k >= 1: key[k] < key[k - 1] (descents) and
//                     key[k] == key[k - 1] (adjacent repeats).  The host reads the record back ONCE, here.
//                       descents == 0                  the sort is skipped (0 sort passes)
//                       descents == repeats == 0       the summation is skipped too, no map is kept, values are used where they lie
//   2. stable LSD radix sort of the keys by 8-bit digits, the entry's position as payload; only the digits that cover bits in use
//      run: ceil(ceil(log2 n) / 8) per field.  Per pass three kinds of launches -- k_coo_hist (digit counts per tile of COO_TILE
//      entries), an exclusive scan of the [digit][tile] table (k_scan_reduce / k_scan_top / k_scan_apply), k_coo_scatter --
//      and workgroups exchange data across launch boundaries only: nothing waits on a word another workgroup writes.  The rank of
//      an entry inside its tile comes from wave ballots and LDS counts taken in input order; no global atomic is on that path.
//   3. heads and compress: a sorted position is a head when its key differs from its predecessor's.  The exclusive scan of the
//      head flags (the same three scan launches, the flags computed from the keys on the fly) gives the stored entry e of every
//      head: colind[e], seg[e]; seg[nnz_stored] = nnz.  k_coo_rowptr then finds rowptr[i], i <= n, by bisection over the stored
//      entries' rows: one thread per ROW, so empty rows -- leading, trailing, runs of them -- need no special case.
//   4. k_coo_segsum   out[e] = sum of vals[src[p]], p = seg[e] .. seg[e + 1] - 1, left to right.  One lane per segment up to
//                     COO_LONG entries.  Longer segments are then taken by the whole wave, one after the other: the lanes gather
//                     64 values at a time (the loads of a chunk are independent of each other) and every lane adds them in order
//                     from the wave's registers.  A segment of L entries so costs L dependent ADDS, not L dependent gathers:
//                     the order contract allows no less, and a wave is busy for at most the entries of its own 64 segments.
//
// Unchecked values.  Every launch after k_coo_key is issued behind the status read-back, i.e. only for indices in [0, n).
// k_coo_key itself indexes by positions only.  (The radix digits are masked, the scatter addresses come from counts of those
// digits, and rowptr is written per row index -- so even these launches index by nothing a bad input could push out of bounds.)
//
// Memory.  Temporary, released before return: two key buffers (8 nnz each), two payload buffers (4 nnz each) -- one key buffer
// and no payload when the sort is skipped --, the [256][tiles] digit table and the scan partials (4 (256 tiles + tiles / 8)),
// the summed values.  Kept on the operator for expv_mi_op_update_values, only when a coordinate repeats or the sort ran:
// src[nnz] (sorted position -> caller position, int32; absent when the sort was skipped) and seg[nnz_stored + 1] (int32).
#include <cstdint>
#include <stdexcept>
#include <string>

#include "kernel_common.h"

namespace expv_mi {
namespace dev {

namespace {
typedef unsigned long long ull;
constexpr ull NOPOS = ~0ull;
constexpr int COO_TILE = 2048;                      // entries a workgroup ranks and scatters per sort pass
constexpr int COO_ROUNDS = COO_TILE / BLOCK;        // ... in rounds of one entry per thread, in input order
constexpr int COO_LONG = 32;                        // segments longer than this are summed by the whole wave
constexpr int SCAN_ITEMS = 8;                       // consecutive items of a thread in the scans
constexpr int SCAN_TILE = SCAN_ITEMS * BLOCK;
constexpr int RADIX = 256;

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
// totals of the workgroup in thread 0 (flags: or; the two positions: min; the two counts: sum) -> the status record
__device__ __forceinline__ void publish(ull flags, ull prow, ull pcol, ull desc, ull eq, CooStatus *st) {
  __shared__ ull sh[5][BLOCK / 64];
  flags = wave_or(flags);
  prow = wave_min(prow);
  pcol = wave_min(pcol);
  desc = wave_add(desc);
  eq = wave_add(eq);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][w] = flags; sh[1][w] = prow; sh[2][w] = pcol; sh[3][w] = desc; sh[4][w] = eq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < BLOCK / 64; ++q) {
      flags |= sh[0][q];
      prow = sh[1][q] < prow ? sh[1][q] : prow;
      pcol = sh[2][q] < pcol ? sh[2][q] : pcol;
      desc += sh[3][q];
      eq += sh[4][q];
    }
    if (flags) atomicOr(&st->flags, flags);
    if (prow != NOPOS) atomicMin(&st->first_row, prow);
    if (pcol != NOPOS) atomicMin(&st->first_col, pcol);
    if (desc) atomicAdd(&st->descents, desc);
    if (eq) atomicAdd(&st->repeats, eq);
  }
}

// ---- 1. check and key ---------------------------------------------------------------------------------------------------------
template <class I> struct Quad { I v[4]; };
template <class I>
__device__ __forceinline__ Quad<I> load4(const I *p, bool vec) {
  Quad<I> q;
  if (vec) {      // 16-byte loads: one for four 4-byte indices, two for four 8-byte ones
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
__device__ __forceinline__ ull make_key(int64_t r, int64_t c) { return ((ull)(uint32_t)r << 32) | (ull)(uint32_t)c; }

template <class I>
__global__ __launch_bounds__(BLOCK) void k_coo_key(const I *__restrict__ row, const I *__restrict__ col, int64_t n, int64_t nnz, int64_t base,
                                                   bool vec_row, bool vec_col, ull *__restrict__ key, CooStatus *st) {
  ull flags = 0, prow = NOPOS, pcol = NOPOS, desc = 0, eq = 0;
  for (int64_t k = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 4; k < nnz; k += (int64_t)gridDim.x * BLOCK * 4) {
    Quad<I> qr, qc;
    const int len = nnz - k >= 4 ? 4 : (int)(nnz - k);
    if (len == 4) {
      qr = load4<I>(row + k, vec_row);
      qc = load4<I>(col + k, vec_col);
    } else {
      for (int z = 0; z < 4; ++z) { qr.v[z] = z < len ? row[k + z] : (I)base; qc.v[z] = z < len ? col[k + z] : (I)base; }
    }
    // the neighbouring lane's last entry (a cache hit); position 0 has no predecessor
    ull prev = k > 0 ? make_key((int64_t)row[k - 1] - base, (int64_t)col[k - 1] - base) : 0;
    ull o[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) {
      const int64_t r = (int64_t)qr.v[z] - base, c = (int64_t)qc.v[z] - base;
      o[z] = make_key(r, c);
      if (z < len) {
        if (r < 0 || r >= n) { flags |= COO_BAD_ROW; prow = prow < (ull)(k + z) ? prow : (ull)(k + z); }
        if (c < 0 || c >= n) { flags |= COO_BAD_COL; pcol = pcol < (ull)(k + z) ? pcol : (ull)(k + z); }
        if (k + z > 0) { desc += o[z] < prev; eq += o[z] == prev; }
        prev = o[z];
      }
    }
    if (len == 4) {      // (key: the library's buffer, 16-byte aligned)
      ulonglong2 *k2 = reinterpret_cast<ulonglong2 *>(key + k);
      k2[0] = make_ulonglong2(o[0], o[1]);
      k2[1] = make_ulonglong2(o[2], o[3]);
    } else {
      for (int z = 0; z < len; ++z) key[k + z] = o[z];
    }
  }
  publish(flags, prow, pcol, desc, eq, st);
}

// ---- exclusive scan of L 32-bit counts in three launches -------------------------------------------------------------------------
// Src: item i -> its count.  Sink: (item, count, exclusive prefix).  Tiles of SCAN_TILE items, SCAN_ITEMS consecutive ones per thread.
struct ArrSrc {
  const uint32_t *a;
  __device__ __forceinline__ uint32_t operator()(int64_t i) const { return a[i]; }
};
struct HeadSrc {      // 1 where a sorted position starts a new coordinate
  const ull *key;
  __device__ __forceinline__ uint32_t operator()(int64_t q) const { return q == 0 || key[q] != key[q - 1]; }
};
struct ArrSink {      // in place: every thread has read its items before it writes them
  uint32_t *a;
  __device__ __forceinline__ void operator()(int64_t i, uint32_t, uint32_t prefix) const { a[i] = prefix; }
};
struct HeadSink {     // stored entry e = prefix of a head: its column, where its segment starts; the closing seg[nnz_stored] = L
  const ull *key;
  int32_t *colind, *seg;
  int64_t L;
  __device__ __forceinline__ void operator()(int64_t q, uint32_t head, uint32_t prefix) const {
    if (head) {
      colind[prefix] = (int32_t)(uint32_t)key[q];
      seg[prefix] = (int32_t)q;
    }
    if (q == L - 1) seg[prefix + head] = (int32_t)L;
  }
};

// sum of `v` over the workgroup, in every thread
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *sh /* [BLOCK / 64] */) {
  v = (uint32_t)wave_add(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
  for (int q = 0; q < BLOCK / 64; ++q) t += sh[q];
  __syncthreads();
  return t;
}
// exclusive prefix of `v` over the workgroup in thread order
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t *sh /* [BLOCK / 64] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int q = 0; q < w; ++q) before += sh[q];
  __syncthreads();
  return before + inc - v;
}

template <class Src>
__global__ __launch_bounds__(BLOCK) void k_scan_reduce(Src src, int64_t L, uint32_t *__restrict__ part) {
  __shared__ uint32_t sh[BLOCK / 64];
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t s = 0;
#pragma unroll
  for (int z = 0; z < SCAN_ITEMS; ++z)
    if (i0 + z < L) s += src(i0 + z);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// one workgroup: part[0 .. nb) -> its exclusive prefixes, in place; the total -> *total (may be null)
__global__ __launch_bounds__(BLOCK) void k_scan_top(uint32_t *__restrict__ part, int64_t nb, ull *total) {
  __shared__ uint32_t sh[BLOCK / 64];
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += SCAN_TILE) {
    const int64_t i0 = b0 + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int z = 0; z < SCAN_ITEMS; ++z) { v[z] = i0 + z < nb ? part[i0 + z] : 0u; s += v[z]; }
    uint32_t pre = carry + block_excl(s, sh);
#pragma unroll
    for (int z = 0; z < SCAN_ITEMS; ++z) {
      if (i0 + z < nb) part[i0 + z] = pre;
      pre += v[z];
    }
    carry += block_sum(s, sh);
  }
  if (threadIdx.x == 0 && total) *total = carry;
}
template <class Src, class Sink>
__global__ __launch_bounds__(BLOCK) void k_scan_apply(Src src, int64_t L, const uint32_t *__restrict__ part, Sink sink) {
  __shared__ uint32_t sh[BLOCK / 64];
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int z = 0; z < SCAN_ITEMS; ++z) { v[z] = i0 + z < L ? src(i0 + z) : 0u; s += v[z]; }
  uint32_t pre = part[blockIdx.x] + block_excl(s, sh);
#pragma unroll
  for (int z = 0; z < SCAN_ITEMS; ++z) {
    if (i0 + z < L) sink(i0 + z, v[z], pre);
    pre += v[z];
  }
}
int64_t scan_blocks(int64_t L) { return (L + SCAN_TILE - 1) / SCAN_TILE; }
// part: scan_blocks(L) words
template <class Src, class Sink>
void exclusive_scan(hipStream_t s, Src src, Sink sink, int64_t L, uint32_t *part, ull *total) {
  const int64_t nb = scan_blocks(L);
  hipLaunchKernelGGL(k_scan_reduce<Src>, dim3((unsigned)nb), dim3(BLOCK), 0, s, src, L, part);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(BLOCK), 0, s, part, nb, total);
  hipLaunchKernelGGL((k_scan_apply<Src, Sink>), dim3((unsigned)nb), dim3(BLOCK), 0, s, src, L, (const uint32_t *)part, sink);
}

// ---- 2. one pass of the radix sort -----------------------------------------------------------------------------------------------
// hist[d * ntiles + t] = entries of tile t whose digit is d (LDS integer counts: order-free, exact)
__global__ __launch_bounds__(BLOCK) void k_coo_hist(const ull *__restrict__ key, int64_t nnz, int shift, int64_t ntiles, uint32_t *__restrict__ hist) {
  __shared__ uint32_t cnt[RADIX];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t k0 = (int64_t)blockIdx.x * COO_TILE;
  for (int r = 0; r < COO_ROUNDS; ++r) {
    const int64_t k = k0 + r * BLOCK + threadIdx.x;
    if (k < nnz) atomicAdd(&cnt[(uint32_t)(key[k] >> shift) & (RADIX - 1)], 1u);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}
// hist now holds the exclusive scan: where the first entry of (digit, tile) goes.  An entry's rank among the entries of its
// tile with the same digit, IN INPUT ORDER: rounds in order (a running count per digit), inside a round waves in order (a count
// per wave and digit), inside a wave lanes in order (ballots over the 8 bits of the digit).
__global__ __launch_bounds__(BLOCK) void k_coo_scatter(const ull *__restrict__ key_in, const int32_t *__restrict__ pay_in, int64_t nnz, int shift,
                                                       int64_t ntiles, const uint32_t *__restrict__ hist, ull *__restrict__ key_out,
                                                       int32_t *__restrict__ pay_out) {
  static_assert(BLOCK == RADIX, "one thread per digit");
  __shared__ uint32_t run[RADIX], wcnt[BLOCK / 64][RADIX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  run[threadIdx.x] = hist[(int64_t)threadIdx.x * ntiles + blockIdx.x];
  for (int q = 0; q < BLOCK / 64; ++q) wcnt[q][threadIdx.x] = 0;
  __syncthreads();
  const int64_t k0 = (int64_t)blockIdx.x * COO_TILE;
  for (int r = 0; r < COO_ROUNDS; ++r) {
    const int64_t k = k0 + r * BLOCK + threadIdx.x;
    const bool live = k < nnz;
    const ull ky = live ? key_in[k] : 0ull;
    const uint32_t d = (uint32_t)(ky >> shift) & (RADIX - 1);
    ull same = __ballot(live);      // lanes of the wave with a live entry of the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const ull m = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? m : ~m;
    }
    const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (live && below == 0) wcnt[w][d] = (uint32_t)__popcll(same);      // (the first lane of the group)
    __syncthreads();
    if (live) {
      uint32_t pos = run[d] + below;
      for (int q = 0; q < w; ++q) pos += wcnt[q][d];
      key_out[pos] = ky;
      pay_out[pos] = pay_in ? pay_in[k] : (int32_t)k;      // (first pass: the payload is the position itself)
    }
    __syncthreads();
    uint32_t add = 0;
    for (int q = 0; q < BLOCK / 64; ++q) { add += wcnt[q][threadIdx.x]; wcnt[q][threadIdx.x] = 0; }
    run[threadIdx.x] += add;
    __syncthreads();
  }
}

// ---- 3. rowptr by bisection over the stored entries' rows ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_coo_rowptr(const ull *__restrict__ key, const int32_t *__restrict__ seg, int64_t nstored, int64_t n,
                                                      int32_t *__restrict__ rowptr) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i <= n; i += (int64_t)gridDim.x * BLOCK) {
    int64_t lo = 0, hi = nstored;      // first stored entry whose row is >= i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)(key[seg[mid]] >> 32) < i) lo = mid + 1;
      else hi = mid;
    }
    rowptr[i] = (int32_t)lo;
  }
}

// ---- 4. segment sums, left to right ------------------------------------------------------------------------------------------------
// (a caller's array is 8-byte aligned at least: the 16-byte complex type is read by its parts)
template <class T> __device__ __forceinline__ T load_val(const T *p, int64_t i) {
  using R = typename ST<T>::real_t;
  const R *r = reinterpret_cast<const R *>(p);
  T v;
  if constexpr (ST<T>::is_complex) { v.re = r[2 * i]; v.im = r[2 * i + 1]; }
  else v = r[i];
  return v;
}
template <class T>
__global__ __launch_bounds__(BLOCK) void k_coo_segsum(const T *__restrict__ vals, const int32_t *__restrict__ src, const int32_t *__restrict__ seg,
                                                      int64_t nstored, T *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;      // (a wave stays whole: the long form below needs every lane)
  const int64_t s0 = e < nstored ? seg[e] : 0, len = e < nstored ? seg[e + 1] - s0 : 0;
  if (len > 0 && len <= COO_LONG) {
    T acc = load_val(vals, src ? (int64_t)src[s0] : s0);
    for (int64_t p = s0 + 1; p < s0 + len; ++p) acc = ST<T>::add(acc, load_val(vals, src ? (int64_t)src[p] : p));
    out[e] = acc;
  }
  ull todo = __ballot(len > COO_LONG);
  while (todo) {
    const int who = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t b = __shfl(s0, who, 64), L = __shfl(len, who, 64);
    T acc = ST<T>::zero();
    for (int64_t c = 0; c < L; c += 64) {
      const int m = L - c >= 64 ? 64 : (int)(L - c);
      T v = ST<T>::zero();
      if (lane < m) v = load_val(vals, src ? (int64_t)src[b + c + lane] : b + c + lane);
      for (int j = 0; j < m; ++j) {
        const T x = shfl_T<T>(v, j);
        acc = (c == 0 && j == 0) ? x : ST<T>::add(acc, x);
      }
    }
    if (lane == who) out[e] = acc;
  }
}

void check_launch(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(who) + ": " + hipGetErrorString(e));
}
}  // namespace

int coo_tile() { return COO_TILE; }

void coo_keys(hipStream_t s, int idx_bytes, const void *row, const void *col, int64_t n, int64_t nnz, int base, unsigned long long *key,
              CooStatus *st) {
  if (idx_bytes != 4 && idx_bytes != 8) throw std::runtime_error("coo_keys: idx_bytes must be 4 or 8");
  if (n < 0 || nnz < 0 || (reinterpret_cast<uintptr_t>(key) & 15u) != 0) throw std::runtime_error("coo_keys: bad n / nnz / output alignment");
  // the record: flags and counts 0, first offending positions "none"
  if (hipMemsetAsync(st, 0, sizeof(CooStatus), s) != hipSuccess || hipMemsetAsync(&st->first_row, 0xff, 2 * sizeof(ull), s) != hipSuccess)
    throw std::runtime_error("coo_keys: hipMemsetAsync failed");
  if (nnz > 0) {
    const dim3 g(grid_for(nnz, BLOCK * 16));
    const bool vr = (reinterpret_cast<uintptr_t>(row) & 15u) == 0, vc = (reinterpret_cast<uintptr_t>(col) & 15u) == 0;
    if (idx_bytes == 8)
      hipLaunchKernelGGL(k_coo_key<int64_t>, g, dim3(BLOCK), 0, s, static_cast<const int64_t *>(row), static_cast<const int64_t *>(col), n, nnz,
                         (int64_t)base, vr, vc, key, st);
    else
      hipLaunchKernelGGL(k_coo_key<int32_t>, g, dim3(BLOCK), 0, s, static_cast<const int32_t *>(row), static_cast<const int32_t *>(col), n, nnz,
                         (int64_t)base, vr, vc, key, st);
  }
  check_launch("coo_keys");
}

int64_t coo_hist_words(int64_t nnz) {
  const int64_t ntiles = (nnz + COO_TILE - 1) / COO_TILE;
  return RADIX * ntiles + scan_blocks(RADIX * ntiles);
}
int64_t coo_scan_words(int64_t nnz) { return scan_blocks(nnz); }

int coo_sort(hipStream_t s, int64_t n, int64_t nnz, unsigned long long *key[2], int32_t *pay[2], uint32_t *hist) {
  int bits = 0;
  while (bits < 32 && ((int64_t)1 << bits) < n) ++bits;      // bits of n - 1: what either field uses
  const int64_t ntiles = (nnz + COO_TILE - 1) / COO_TILE;
  uint32_t *part = hist + RADIX * ntiles;
  int passes = 0;
  for (int field = 0; field < 2; ++field)
    for (int sh = 0; sh < bits; sh += 8) {
      const int in = passes & 1, shift = 32 * field + sh;
      hipLaunchKernelGGL(k_coo_hist, dim3((unsigned)ntiles), dim3(BLOCK), 0, s, (const ull *)key[in], nnz, shift, ntiles, hist);
      exclusive_scan(s, ArrSrc{hist}, ArrSink{hist}, RADIX * ntiles, part, (ull *)nullptr);
      hipLaunchKernelGGL(k_coo_scatter, dim3((unsigned)ntiles), dim3(BLOCK), 0, s, (const ull *)key[in], (const int32_t *)(passes ? pay[in] : nullptr),
                         nnz, shift, ntiles, (const uint32_t *)hist, key[in ^ 1], pay[in ^ 1]);
      ++passes;
    }
  check_launch("coo_sort");
  return passes;
}

void coo_count_heads(hipStream_t s, const unsigned long long *key, int64_t nnz, uint32_t *part, CooStatus *st) {
  const int64_t nb = scan_blocks(nnz);
  hipLaunchKernelGGL(k_scan_reduce<HeadSrc>, dim3((unsigned)nb), dim3(BLOCK), 0, s, HeadSrc{key}, nnz, part);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(BLOCK), 0, s, part, nb, &st->stored);
  check_launch("coo_count_heads");
}

void coo_compress(hipStream_t s, const unsigned long long *key, int64_t n, int64_t nnz, int64_t nstored, const uint32_t *part, int32_t *rowptr,
                  int32_t *colind, int32_t *seg) {
  if ((reinterpret_cast<uintptr_t>(colind) & 15u) != 0) throw std::runtime_error("coo_compress: bad output alignment");
  hipLaunchKernelGGL((k_scan_apply<HeadSrc, HeadSink>), dim3((unsigned)scan_blocks(nnz)), dim3(BLOCK), 0, s, HeadSrc{key}, nnz, part,
                     HeadSink{key, colind, seg, nnz});
  hipLaunchKernelGGL(k_coo_rowptr, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, s, key, (const int32_t *)seg, nstored, n, rowptr);
  check_launch("coo_compress");
}

template <class T>
void coo_segment_sums(hipStream_t s, const T *vals, const int32_t *src, const int32_t *seg, int64_t nstored, T *out) {
  if (nstored <= 0) return;
  hipLaunchKernelGGL(k_coo_segsum<T>, dim3((unsigned)((nstored + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, vals, src, seg, nstored, out);
  check_launch("coo_segment_sums");
}
template void coo_segment_sums<double>(hipStream_t, const double *, const int32_t *, const int32_t *, int64_t, double *);
template void coo_segment_sums<cplx>(hipStream_t, const cplx *, const int32_t *, const int32_t *, int64_t, cplx *);
template void coo_segment_sums<float>(hipStream_t, const float *, const int32_t *, const int32_t *, int64_t, float *);
template void coo_segment_sums<cplx32>(hipStream_t, const cplx32 *, const int32_t *, const int32_t *, int64_t, cplx32 *);

}  // namespace dev
}  // namespace expv_mi
