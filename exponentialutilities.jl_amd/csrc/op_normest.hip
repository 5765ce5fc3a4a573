// op_normest.hip -- a lower bound of || (A - sigma I)^p ||_1 (or _inf) of a stored operator without forming a power: the block
// 1-norm estimator of Higham & Tisseur (SIAM J. Matrix Anal. Appl. 21, 2000, Algorithm 2.4) with t = 2 columns and itmax = 5, in
// the control flow of scipy's _onenormest_core, made deterministic.  What the truncated-Taylor parameter search needs to take the
// second branch of the reference (ext/ExponentialUtilitiesStaticArraysExt.jl:104-121), which forms A^2, A^3, ... densely.
//
//   forward leg   Y = M X,  M = (A - sigma I)^p: p applications of the operator to the two columns
//   the host reads the column sums sum_i |y_ik| (and, for the real types, the counts of agreeing signs), decides
//   backward leg  Z = M' S, S = sign(Y): p applications of the ADJOINT operator
//   the host reads the 12 largest h_i = max_k |z_ik| with their natural indices, decides, X = two unit vectors
//
// The infinity norm of B^p is the 1-norm of (B')^p: `which` swaps the two operators and conjugates the shift.
//
// Deterministic: column 0 starts as 1/n, every "random" sign is normest_sign(natural row, column, draw) (mix64.h), every tie goes
// to the smaller natural index, column sums are fp64 per-workgroup partials finished in index order by the workgroup that arrives
// last, the parallel-column tests are integer counts.  Vectors cross a leg boundary in the caller's natural ordering: an operator
// stored as P A P' gets its columns gathered in at the start of its leg and out at its end.
//
// No overflow, no underflow: every application leaves the maxima of its output columns on the device (integer atomic maxima of
// non-negative bit patterns), and the NEXT application multiplies its result by the exact power of two that would have brought
// its input column into [1, 2): (A x - sigma x) 2^-e = (A - sigma I)(x 2^-e) bit for bit.  The exponents are summed per column in
// integers -- by the host for the column sums, by the selection kernel for h -- so the estimate of 2^k A is 2^(kp) times the
// estimate of A with the same mantissa.  The measure of a complex column is max(|re|, |im|): exact, in [1, 2) after scaling while
// the moduli stay below 2 sqrt 2.  The scale is applied to the result, not to x as it is loaded: the accumulator A x - sigma x holds
// two applications' growth before it is scaled, so the range is ||B|| in about 2^-63 .. 2^63 for the 32-bit types.
//
// The panel apply.  An operator with a fused form (taylor_fused: SELL slots without overflow entries, or the general diagonal form)
// takes the row walk of the block term kernel (sparse_rows.h) on [row][P] interleaved columns, P = 2 for the 64-bit types and for
// ComplexF32, 4 for Float32 (the smallest whole 16-byte pack; the padding columns are zero and take no part in a maximum): the
// operator is read once for both columns, and the shift, the scaling and the maxima ride in the same pass.  A leg packs its start
// columns into the panel (the gather into the operator's stored ordering in the same pass) and unpacks its result.  Every other
// operator goes column by column through op_apply_dev plus an update kernel on 16-byte packs, the split expv_taylor_block makes.
// Launches follow each other on the stream, no kernel waits for another.  gfx950 only.
#include <algorithm>
#include <climits>
#include <cmath>
#include <complex>
#include <cstring>
#include <limits>
#include <vector>

#include "engine.h"
#include "kernel_common.h"
#include "mix64.h"
#include "sparse_rows.h"
#include "taylor_state.h"
#include "taylor_term.h"

namespace expv_mi {
namespace dev {

constexpr int NE_COLS = 2, NE_PMAX = 16, NE_TOP = 12;

// One leg's state.  colmax[k][a]: bit pattern of the maximum of the input column k of application a (a = 0: written by the kernel
// that made the leg's start vectors), [p] of the leg's result.  agree: S_k against Sold_j at [2 k + j], S_0 against S_1 at [4].
struct NeState {
  unsigned long long colmax[NE_COLS][NE_PMAX + 2];
  unsigned long long agree[8];
  unsigned long long ticket, nan;
  double colsum[NE_COLS];
  double topval[NE_TOP];
  long long topidx[NE_TOP];
  long long emax;
  unsigned long long pad[5];
};
static_assert(sizeof(NeState) % 16 == 0, "NeState layout");

}  // namespace dev

// floor(log2 m) of a column maximum given as its bit pattern, clamped to what the real type can scale by; 0 for a zero, subnormal
// or non-finite maximum (such a column is not scaled)
__host__ __device__ static inline int ne_exponent(unsigned long long bits, int lim) {
  const int f = (int)((bits >> 52) & 0x7ffull);
  if (f == 0 || f == 0x7ff) return 0;
  const int e = f - 1023;
  return e < -lim ? -lim : (e > lim ? lim : e);
}
__host__ __device__ static inline double ne_pow2(int e) {
  const unsigned long long b = (unsigned long long)(1023 + e) << 52;
  double d;
#if defined(__HIP_DEVICE_COMPILE__)
  d = __longlong_as_double((long long)b);
#else
  std::memcpy(&d, &b, 8);
#endif
  return d;
}
template <class T> constexpr int ne_lim() { return sizeof(typename ST<T>::real_t) == 4 ? 126 : 1022; }

namespace dev {

__device__ __forceinline__ double ne_measure(double v) { return fabs(v); }
__device__ __forceinline__ double ne_measure(float v) { return (double)fabsf(v); }
__device__ __forceinline__ double ne_measure(cplx v) { return fmax(fabs(v.re), fabs(v.im)); }
__device__ __forceinline__ double ne_measure(cplx32 v) { return (double)fmaxf(fabsf(v.re), fabsf(v.im)); }

// the workgroup's maxima of two columns into their words; NaN flags into st->nan
__device__ __forceinline__ void ne_block_max(double m0, double m1, unsigned nan, unsigned long long *w0, unsigned long long *w1, NeState *st) {
  __shared__ double m0_s[BLOCK / 64], m1_s[BLOCK / 64];
  __shared__ unsigned nan_s[BLOCK / 64];
  m0 = wave_max(m0);
  m1 = wave_max(m1);
  nan = __any((int)nan) ? 1u : 0u;
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { m0_s[wave] = m0; m1_s[wave] = m1; nan_s[wave] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) { m0 = fmax(m0, m0_s[w]); m1 = fmax(m1, m1_s[w]); nan |= nan_s[w]; }
    if (m0 > 0.0) atomicMax(w0, (unsigned long long)__double_as_longlong(m0));
    if (m1 > 0.0) atomicMax(w1, (unsigned long long)__double_as_longlong(m1));
    if (nan) atomicOr(&st->nan, 1ull);
  }
}

// true in the workgroup that arrives last (every store of the others was performed before their tickets)
__device__ __forceinline__ bool ne_last_block(NeState *st) {
  __shared__ int last_s;
  __syncthreads();
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __hip_atomic_fetch_add(&st->ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = (t == (unsigned long long)gridDim.x - 1ull);
  }
  __syncthreads();
  return last_s != 0;
}

// ---- start vectors ----
// mode 0: X_0 = 1/n, X_1 = +-1/n by normest_sign(i, 1, attempt);  mode 1: X_k = e_{ind_k} (ind_k < 0: the zero column)
template <class T>
__global__ __launch_bounds__(BLOCK) void k_ne_start(int mode, T *x0, T *x1, int64_t n, double inv_n, unsigned attempt, long long ind0, long long ind1,
                                                   NeState *st) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    if (mode == 0) {
      x0[i] = ST<T>::from_real(inv_n);
      x1[i] = ST<T>::from_real(normest_sign((uint64_t)i, 1u, attempt) > 0 ? inv_n : -inv_n);
    } else {
      x0[i] = ST<T>::from_real(i == ind0 ? 1.0 : 0.0);
      x1[i] = ST<T>::from_real(i == ind1 ? 1.0 : 0.0);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double m0 = mode == 0 ? (double)ST<T>::real(ST<T>::from_real(inv_n)) : (ind0 >= 0 ? 1.0 : 0.0);
    const double m1 = mode == 0 ? m0 : (ind1 >= 0 ? 1.0 : 0.0);
    ts_storef(&st->colmax[0][0], m0);
    ts_storef(&st->colmax[1][0], m1);
  }
}

// ---- one application, behind y_k = A x_k:  y_k <- (y_k - sigma x_k) 2^-e_k, e_k from the maximum of x_k; maxima of the result ----
template <class T>
struct NeUpdArgs {
  const T *x[NE_COLS];
  T *y[NE_COLS];
  int64_t n;
  T sigma;
  int a;
  NeState *st;
};
template <class T>
__global__ __launch_bounds__(BLOCK) void k_ne_update(NeUpdArgs<T> g) {
  constexpr int N = Pack<T>::N;
  double sc[NE_COLS], m[NE_COLS] = {0.0, 0.0};
  unsigned nan = 0u;
#pragma unroll
  for (int k = 0; k < NE_COLS; ++k) sc[k] = ne_pow2(-ne_exponent(ts_load(&g.st->colmax[k][g.a]), ne_lim<T>()));
  for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * N; i < g.n; i += (int64_t)gridDim.x * BLOCK * N) {
#pragma unroll
    for (int k = 0; k < NE_COLS; ++k) {
      const bool alx = is_al16(g.x[k]), aly = is_al16(g.y[k]);
      const Pack<T> xi = ld_pack_user(g.x[k], i, g.n, alx);
      Pack<T> yi = ld_pack_user(g.y[k], i, g.n, aly);
#pragma unroll
      for (int q = 0; q < N; ++q) {
        T v = yi.v[q];
        ST<T>::nfma(v, g.sigma, xi.v[q]);
        v = ST<T>::mul_real(v, sc[k]);
        yi.v[q] = v;
        if (i + q < g.n) note_abs(ne_measure(v), m[k], nan, 1u);
      }
      st_pack_user(g.y[k], i, g.n, aly, yi);
    }
  }
  ne_block_max(m[0], m[1], nan, &g.st->colmax[0][g.a + 1], &g.st->colmax[1][g.a + 1], g.st);
}

// ---- the same application in one pass over an operator with a fused form, on [row][P] interleaved columns ----
template <class T> struct NePanel { static constexpr int P = sizeof(T) == 4 ? 4 : 2; };

// X[r][k] = in_k[perm ? perm[r] : r] for r < n, zero in the padding rows and columns
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_ne_pack(const T *__restrict__ in0, const T *__restrict__ in1, const int32_t *__restrict__ perm, T *X, int64_t n,
                                                  int64_t rows) {
  using Row = RowP<T, P>;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * BLOCK) {
    Row x = BlockColumns<T, P>::none();
    if (r < n) {
      const int64_t src = perm ? (int64_t)perm[r] : r;
      x.v[0] = in0[src];
      x.v[1] = in1[src];
    }
    *reinterpret_cast<Row *>(X + r * P) = x;
  }
}
// out_k[i] = Y[pinv ? pinv[i] : i][k], i < n
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_ne_unpack(const T *__restrict__ Y, const int32_t *__restrict__ pinv, T *out0, T *out1, int64_t n) {
  using Row = RowP<T, P>;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    const int64_t r = pinv ? (int64_t)pinv[i] : i;
    const Row y = *reinterpret_cast<const Row *>(Y + r * P);
    out0[i] = y.v[0];
    out1[i] = y.v[1];
  }
}
template <class T>
struct NePanelArgs {
  TaylorOpView<T> op;
  const T *x;      // [rows][P], rows = whole slices
  T *y;
  int64_t n;
  T sigma;
  int a;
  NeState *st;
};
// the lane <-> row mapping of k_taylor_term_block: one 16-byte row pack of the operator per lane, whole slices
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_ne_apply_panel(NePanelArgs<T> g) {
  constexpr int N = Pack<T>::N;
  constexpr int SH = 64 * N;
  using Row = RowP<T, P>;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nsl = (g.n + SH - 1) / SH;
  double sc[NE_COLS], m[NE_COLS] = {0.0, 0.0};
  unsigned nan = 0u;
#pragma unroll
  for (int k = 0; k < NE_COLS; ++k) sc[k] = ne_pow2(-ne_exponent(ts_load(&g.st->colmax[k][g.a]), ne_lim<T>()));
  for (int64_t slice = (int64_t)blockIdx.x * (BLOCK / 64) + wave; slice < nsl; slice += (int64_t)gridDim.x * (BLOCK / 64)) {
    const int64_t i = slice * SH + (int64_t)lane * N;
    T acc[N][P];
    BlockColumns<T, P> xs{g.x, acc};
    if (g.op.ndiag > 0) dia_walk<T, 4>(g.op.dia_val, g.op.dia_ld, g.op.ndiag, g.op.dia_off, i, g.n, xs);
    else sell_walk<T, 4>(g.op.A, slice, lane, xs);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const Row xi = *reinterpret_cast<const Row *>(g.x + (i + q) * P);
      Row y = BlockColumns<T, P>::none();
#pragma unroll
      for (int k = 0; k < NE_COLS; ++k) {
        T v = acc[q][k];
        ST<T>::nfma(v, g.sigma, xi.v[k]);
        v = ST<T>::mul_real(v, sc[k]);
        y.v[k] = v;
        if (i + q < g.n) note_abs(ne_measure(v), m[k], nan, 1u);
      }
      *reinterpret_cast<Row *>(g.y + (i + q) * P) = y;
    }
  }
  ne_block_max(m[0], m[1], nan, &g.st->colmax[0][g.a + 1], &g.st->colmax[1][g.a + 1], g.st);
}

// ---- forward epilogue: colsum_k = sum_i |y_ik| in fp64 ----
template <class T>
__global__ __launch_bounds__(BLOCK) void k_ne_colsum(const T *y0, const T *y1, int64_t n, double *part, NeState *st) {
  __shared__ double red_s[BLOCK / 64];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    s0 += abs_T(y0[i]);
    s1 += abs_T(y1[i]);
  }
  const double b0 = block_sum(s0, red_s);
  __syncthreads();
  const double b1 = block_sum(s1, red_s);
  if (threadIdx.x == 0) {
    publish_f64(part + blockIdx.x, b0);
    publish_f64(part + MAX_GRID + blockIdx.x, b1);
  }
  if (!ne_last_block(st)) return;
  s0 = 0.0;
  s1 = 0.0;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += BLOCK) {
    s0 += consume_f64(part + b);
    s1 += consume_f64(part + MAX_GRID + b);
  }
  __syncthreads();
  s0 = block_sum(s0, red_s);
  __syncthreads();
  s1 = block_sum(s1, red_s);
  if (threadIdx.x == 0) {
    st->colsum[0] = s0;
    st->colsum[1] = s1;
    ts_store(&st->ticket, 0ull);
  }
}

// ---- S = sign(Y), with the counts of agreeing signs (real types) or the maxima of the unit-modulus signs (complex types) ----
// y[0] == nullptr: S is kept as it is (a resampling pass).  resample = k: column k of S becomes normest_sign(i, k, attempt).
template <class T>
struct NeSignArgs {
  const T *y[NE_COLS];
  T *s[NE_COLS];
  const T *so[NE_COLS];
  int64_t n;
  int resample;
  unsigned attempt;
  NeState *fwd, *bwd;      // counts go to the forward leg's state (read with its column sums), maxima start the backward leg
};
template <class T>
__global__ __launch_bounds__(BLOCK) void k_ne_sign(NeSignArgs<T> g) {
  using R = typename ST<T>::real_t;
  if constexpr (ST<T>::is_complex) {
    double m[NE_COLS] = {0.0, 0.0};
    unsigned nan = 0u;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * BLOCK) {
#pragma unroll
      for (int k = 0; k < NE_COLS; ++k) {
        const T y = g.y[k][i];
        const double re = (double)y.re, im = (double)y.im, a = hypot(re, im);
        T s;
        if (a == 0.0) { s.re = (R)1; s.im = (R)0; }
        else { s.re = (R)(re / a); s.im = (R)(im / a); }
        g.s[k][i] = s;
        note_abs(ne_measure(s), m[k], nan, 1u);
      }
    }
    ne_block_max(m[0], m[1], nan, &g.bwd->colmax[0][0], &g.bwd->colmax[1][0], g.bwd);
  } else {
    __shared__ unsigned long long cnt_s[BLOCK / 64][5];
    unsigned long long c[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * BLOCK) {
      T s[NE_COLS];
#pragma unroll
      for (int k = 0; k < NE_COLS; ++k) {
        if (k == g.resample) s[k] = (T)normest_sign((uint64_t)i, (uint32_t)k, g.attempt);
        else if (g.y[0]) s[k] = g.y[k][i] < (T)0 ? (T)-1 : (T)1;
        else s[k] = g.s[k][i];
        if (k == g.resample || g.y[0]) g.s[k][i] = s[k];
        c[2 * k] += s[k] == g.so[0][i] ? 1ull : 0ull;
        c[2 * k + 1] += s[k] == g.so[1][i] ? 1ull : 0ull;
      }
      c[4] += s[0] == s[1] ? 1ull : 0ull;
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      for (int off = 32; off >= 1; off >>= 1) c[q] += __shfl_xor(c[q], off, 64);
      if ((threadIdx.x & 63) == 0) cnt_s[wave][q] = c[q];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
      unsigned long long t = 0ull;
      for (int w = 0; w < BLOCK / 64; ++w) t += cnt_s[w][threadIdx.x];
      if (t) atomicAdd(&g.fwd->agree[threadIdx.x], t);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ts_storef(&g.bwd->colmax[0][0], 1.0);
      ts_storef(&g.bwd->colmax[1][0], 1.0);
    }
  }
}

// ---- backward epilogue: the NE_TOP largest h_i = max_k |z_ik| 2^(E_k - max E), ties to the smaller index ----
__device__ __forceinline__ bool ne_better(double v, long long i, double w, long long j) { return v > w || (v == w && i < j); }

struct NeList {
  double v[NE_TOP];
  long long i[NE_TOP];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < NE_TOP; ++q) { v[q] = -1.0; i[q] = LLONG_MAX; }
  }
  __device__ __forceinline__ void offer(double w, long long j) {      // the list stays sorted, best first
#pragma unroll
    for (int q = NE_TOP - 1; q >= 0; --q) {
      if (ne_better(w, j, v[q], i[q])) {
        if (q < NE_TOP - 1) { v[q + 1] = v[q]; i[q + 1] = i[q]; }
        v[q] = w; i[q] = j;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int q = 0; q < NE_TOP - 1; ++q) { v[q] = v[q + 1]; i[q] = i[q + 1]; }
    v[NE_TOP - 1] = -1.0; i[NE_TOP - 1] = LLONG_MAX;
  }
};
// The workgroup's NE_TOP best of its threads' lists, in order; lane 0 of wave 0 hands each to put(rank, value, index).
template <class P>
__device__ __forceinline__ void ne_block_select(NeList &l, P &&put) {
  __shared__ double bv_s[BLOCK / 64];
  __shared__ long long bi_s[BLOCK / 64];
  const int wave = threadIdx.x >> 6;
  for (int r = 0; r < NE_TOP; ++r) {
    double v = l.v[0];
    long long i = l.i[0];
    for (int off = 32; off >= 1; off >>= 1) {
      const double w = __shfl_xor(v, off, 64);
      const long long j = __shfl_xor(i, off, 64);
      if (ne_better(w, j, v, i)) { v = w; i = j; }
    }
    if ((threadIdx.x & 63) == 0) { bv_s[wave] = v; bi_s[wave] = i; }
    __syncthreads();
    v = bv_s[0];
    i = bi_s[0];
    for (int w = 1; w < BLOCK / 64; ++w)
      if (ne_better(bv_s[w], bi_s[w], v, i)) { v = bv_s[w]; i = bi_s[w]; }
    if (l.v[0] == v && l.i[0] == i) l.pop();
    if (threadIdx.x == 0) put(r, v, i);
    __syncthreads();
  }
}
template <class T>
__global__ __launch_bounds__(BLOCK) void k_ne_top(const T *z0, const T *z1, int64_t n, int p, double *pval, long long *pidx, NeState *st) {
  int E[NE_COLS];
#pragma unroll
  for (int k = 0; k < NE_COLS; ++k) {
    E[k] = 0;
    for (int a = 0; a < p; ++a) E[k] += ne_exponent(ts_load(&st->colmax[k][a]), ne_lim<T>());
  }
  const int emax = E[0] > E[1] ? E[0] : E[1];
  NeList l;
  l.clear();
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    double h = fmax(ldexp(abs_T(z0[i]), E[0] - emax), ldexp(abs_T(z1[i]), E[1] - emax));
    if (h != h) h = 0.0;
    l.offer(h, (long long)i);
  }
  ne_block_select(l, [&](int r, double v, long long i) {
    publish_f64(pval + (size_t)blockIdx.x * NE_TOP + r, v);
    __hip_atomic_store(pidx + (size_t)blockIdx.x * NE_TOP + r, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
  if (!ne_last_block(st)) return;
  l.clear();
  const int ncand = (int)gridDim.x * NE_TOP;
  for (int c = threadIdx.x; c < ncand; c += BLOCK) {
    const double v = consume_f64(pval + c);
    const long long i = __hip_atomic_load(pidx + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    l.offer(v, i);
  }
  ne_block_select(l, [&](int r, double v, long long i) {
    st->topval[r] = v;
    st->topidx[r] = v < 0.0 ? -1ll : i;
  });
  if (threadIdx.x == 0) {
    st->emax = emax;
    ts_store(&st->ticket, 0ull);
  }
}

}  // namespace dev

// ------------------------------------------------------------------------------------------
// the host loop                                   scipy/sparse/linalg/_onenormest.py: _onenormest_core
// ------------------------------------------------------------------------------------------
namespace {

enum { NE_EXIT_NO_GROWTH = 1, NE_EXIT_ITMAX = 2, NE_EXIT_PARALLEL = 3, NE_EXIT_HMAX_IS_BEST = 4, NE_EXIT_VISITED = 5, NE_EXIT_NONFINITE = 6,
       NE_EXIT_EXACT = 7 };
constexpr int NE_ITMAX = 5;

template <class T>
struct NeRun {
  Ctx *c;
  int64_t n;
  int p;
  size_t vbytes;
  DevBuf work;
  T *P[2], *Q[2], *G[2], *S[2], *So[2], *X[2];
  dev::NeState *fwd, *bwd;
  T *XP[2];       // the two panels of a fused leg, [rows][P]
  int64_t rows;   // n rounded up to whole slices
  double *part;
  double *pval;
  long long *pidx;
  int grid, grid_pack, grid_rows, grid_slices;
  int64_t apps = 0, reads = 0;

  NeRun(Ctx *c_, int64_t n_, int p_) : c(c_), n(n_), p(p_) {
    vbytes = up16((size_t)n * sizeof(T)) + 16;
    const size_t sbytes = up16(sizeof(dev::NeState));
    const size_t pbytes = sizeof(double) * 2 * dev::MAX_GRID, tbytes = (size_t)dev::MAX_GRID * dev::NE_TOP * 8;
    constexpr int SH = 64 * dev::Pack<T>::N;
    const int64_t nsl = (n + SH - 1) / SH;
    rows = nsl * SH;
    const size_t xbytes = (size_t)rows * dev::NePanel<T>::P * sizeof(T);
    work.take_from(c, 12 * vbytes + 2 * xbytes + 2 * sbytes + pbytes + 2 * tbytes);
    char *b = work.as<char>();
    for (int k = 0; k < 2; ++k) { XP[k] = reinterpret_cast<T *>(b); b += xbytes; }
    auto vec = [&]() { T *v = reinterpret_cast<T *>(b); b += vbytes; return v; };
    for (int k = 0; k < 2; ++k) { P[k] = vec(); Q[k] = vec(); G[k] = vec(); S[k] = vec(); So[k] = vec(); X[k] = vec(); }
    fwd = reinterpret_cast<dev::NeState *>(b); b += sbytes;
    bwd = reinterpret_cast<dev::NeState *>(b); b += sbytes;
    part = reinterpret_cast<double *>(b); b += pbytes;
    pval = reinterpret_cast<double *>(b); b += tbytes;
    pidx = reinterpret_cast<long long *>(b);
    grid = dev::taylor_grid(n, dev::BLOCK);
    grid_pack = dev::taylor_grid(n, dev::BLOCK * dev::Pack<T>::N);
    grid_rows = dev::taylor_grid(rows, dev::BLOCK);
    grid_slices = dev::taylor_grid(nsl, dev::BLOCK / 64);
  }
  void zero(dev::NeState *st) { HIPCHECK(hipMemsetAsync(st, 0, sizeof(dev::NeState), c->stream)); }

  // M in[k] for the two natural-ordered columns `in`: p applications of `op` with `shift`; the result's natural-ordered columns in out[]
  void leg(Op &op, std::complex<double> shift, T *const in[2], dev::NeState *st, T *out[2]) {
    hipStream_t s = c->stream;
    if (taylor_fused(op)) {
      constexpr int PP = dev::NePanel<T>::P;
      {
        ProfScope ps(c, EXPV_MI_K_LINCOMB);
        hipLaunchKernelGGL((dev::k_ne_pack<T, PP>), dim3(grid_rows), dim3(dev::BLOCK), 0, s, in[0], in[1],
                           op.perm ? op.perm->p.as<int32_t>() : nullptr, XP[0], n, rows);
      }
      dev::NePanelArgs<T> g{};
      g.op = taylor_op_view<T>(c, op);
      g.n = n; g.sigma = taylor_scalar<T>(shift); g.st = st;
      int cur = 0;
      for (int a = 0; a < p; ++a) {
        g.x = XP[cur]; g.y = XP[1 - cur]; g.a = a;
        ++c->cnt_opapply;
        ProfScope ps(c, EXPV_MI_K_MATVEC);
        hipLaunchKernelGGL((dev::k_ne_apply_panel<T, PP>), dim3(grid_slices), dim3(dev::BLOCK), 0, s, g);
        ++apps;
        cur ^= 1;
      }
      ProfScope ps(c, EXPV_MI_K_LINCOMB);
      hipLaunchKernelGGL((dev::k_ne_unpack<T, PP>), dim3(grid), dim3(dev::BLOCK), 0, s, XP[cur], op.perm ? op.perm->pinv.as<int32_t>() : nullptr,
                         P[0], P[1], n);
      out[0] = P[0];
      out[1] = P[1];
      return;
    }
    const T *src[2] = {in[0], in[1]};
    if (op.perm) {
      for (int k = 0; k < 2; ++k) {
        dev::gather_rows(s, sizeof(T), G[k], n, in[k], n, op.perm->p.as<int32_t>(), n, 1);
        src[k] = G[k];
      }
    }
    T *dst[2] = {P[0], P[1]}, *other[2] = {Q[0], Q[1]};
    for (int a = 0; a < p; ++a) {
      for (int k = 0; k < 2; ++k) op_apply_dev(op, src[k], dst[k], nullptr, 0);
      dev::NeUpdArgs<T> g{};
      for (int k = 0; k < 2; ++k) { g.x[k] = src[k]; g.y[k] = dst[k]; }
      g.n = n; g.sigma = taylor_scalar<T>(shift); g.a = a; g.st = st;
      {
        ProfScope ps(c, EXPV_MI_K_LINCOMB);
        hipLaunchKernelGGL(dev::k_ne_update<T>, dim3(grid_pack), dim3(dev::BLOCK), 0, s, g);
      }
      ++apps;
      for (int k = 0; k < 2; ++k) { src[k] = dst[k]; std::swap(dst[k], other[k]); }
    }
    for (int k = 0; k < 2; ++k) {
      if (op.perm) {      // (dst is the buffer the result is not in)
        dev::gather_rows(s, sizeof(T), dst[k], n, src[k], n, op.perm->pinv.as<int32_t>(), n, 1);
        out[k] = dst[k];
      } else {
        out[k] = const_cast<T *>(src[k]);
      }
    }
  }
  void start(int mode, unsigned attempt, long long i0, long long i1) {
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_ne_start<T>, dim3(grid), dim3(dev::BLOCK), 0, c->stream, mode, X[0], X[1], n, 1.0 / (double)n, attempt, i0, i1, fwd);
  }
  void colsum(T *const y[2]) {
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_ne_colsum<T>, dim3(grid), dim3(dev::BLOCK), 0, c->stream, y[0], y[1], n, part, fwd);
  }
  void sign(T *const y[2], int resample, unsigned attempt) {
    HIPCHECK(hipMemsetAsync(fwd->agree, 0, sizeof(fwd->agree), c->stream));
    dev::NeSignArgs<T> g{};
    for (int k = 0; k < 2; ++k) { g.y[k] = y ? y[k] : nullptr; g.s[k] = S[k]; g.so[k] = So[k]; }
    g.n = n; g.resample = resample; g.attempt = attempt; g.fwd = fwd; g.bwd = bwd;
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_ne_sign<T>, dim3(grid), dim3(dev::BLOCK), 0, c->stream, g);
  }
  void top(T *const z[2]) {
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_ne_top<T>, dim3(grid), dim3(dev::BLOCK), 0, c->stream, z[0], z[1], n, p, pval, pidx, bwd);
  }
  void read(dev::NeState *st, dev::NeState &h) {
    HIPCHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    ++reads;
  }
  // sum_i |y_ik| of the leg's result behind the scalings of its p applications
  double column_estimate(const dev::NeState &h, int k) const {
    int E = 0;
    for (int a = 0; a < p; ++a) E += ne_exponent(h.colmax[k][a], ne_lim<T>());
    return std::ldexp(h.colsum[k], E);
  }
};

template <class T>
void normest_T(Ctx *c, Op &A, Op &AH, int p, std::complex<double> sigma, int64_t info[8], double *est_out) {
  constexpr bool is_complex = ST<T>::is_complex;
  const int64_t n = A.n;
  hipStream_t s = c->stream;
  NeRun<T> r(c, n, p);
  const std::complex<double> sigma_h = std::conj(sigma);
  int64_t resamples = 0, ind_best = -1;
  int exit_code = 0, k = 1;
  double est = 0.0, est_old = 0.0;
  T *Y[2], *Z[2];
  dev::NeState h;

  auto finish = [&]() {
    info[0] = k; info[1] = r.apps; info[2] = r.reads; info[3] = ind_best; info[4] = resamples; info[5] = exit_code;
    *est_out = est;
  };

  if (n <= 2) {      // fewer rows than columns + 1: the unit vectors give every column sum
    r.zero(r.fwd);
    r.start(1, 0u, 0, n > 1 ? 1 : -1);
    r.leg(A, sigma, r.X, r.fwd, Y);
    r.colsum(Y);
    r.read(r.fwd, h);
    const double e0 = r.column_estimate(h, 0), e1 = n > 1 ? r.column_estimate(h, 1) : 0.0;
    est = (e1 > e0) ? e1 : e0;
    if (e0 != e0 || e1 != e1) est = std::numeric_limits<double>::quiet_NaN();
    ind_best = (e1 > e0) ? 1 : 0;
    exit_code = NE_EXIT_EXACT;
    finish();
    return;
  }

  // column 1 of the start block: the first draw that is not parallel to the column of ones
  unsigned attempt = 0;
  for (;;) {
    int64_t i = 0;
    while (i < n && normest_sign((uint64_t)i, 1u, attempt) > 0) ++i;
    if (i < n) break;
    ++attempt;
    ++resamples;
  }
  unsigned draws = attempt + 1;      // the next draw's counter
  r.zero(r.fwd);
  r.start(0, attempt, 0, 0);
  HIPCHECK(hipMemsetAsync(r.S[0], 0, r.vbytes, s));      // S_old of the first iteration: parallel to nothing
  HIPCHECK(hipMemsetAsync(r.S[1], 0, r.vbytes, s));

  std::vector<long long> ind, ind_hist;
  for (;;) {
    r.leg(A, sigma, r.X, r.fwd, Y);
    r.colsum(Y);
    for (int q = 0; q < 2; ++q) std::swap(r.S[q], r.So[q]);      // S_old = S;  the new S is queued ahead of the read
    r.zero(r.bwd);
    r.sign(Y, -1, 0u);
    r.read(r.fwd, h);
    const double e0 = r.column_estimate(h, 0), e1 = r.column_estimate(h, 1);
    if (h.nan || !(e0 == e0) || !(e1 == e1)) {
      est = std::numeric_limits<double>::quiet_NaN();
      exit_code = NE_EXIT_NONFINITE;
      break;
    }
    const int best_j = (e1 > e0) ? 1 : 0;
    est = best_j ? e1 : e0;
    if ((est > est_old || k == 2) && k >= 2) ind_best = ind[best_j];
    if (k >= 2 && est <= est_old) { est = est_old; exit_code = NE_EXIT_NO_GROWTH; break; }
    est_old = est;
    if (k > NE_ITMAX) { exit_code = NE_EXIT_ITMAX; break; }
    if (!is_complex) {
      auto par_old = [&](int q) { return h.agree[2 * q] == (unsigned long long)n || h.agree[2 * q + 1] == (unsigned long long)n; };
      if (par_old(0) && par_old(1)) { exit_code = NE_EXIT_PARALLEL; break; }
      for (int q = 0; q < 2; ++q) {
        while (par_old(q) || (q == 1 && h.agree[4] == (unsigned long long)n)) {
          r.sign(nullptr, q, draws++);
          ++resamples;
          r.read(r.fwd, h);      // (one more read per resampled column: the counts of the new column)
        }
      }
    }
    r.leg(AH, sigma_h, r.S, r.bwd, Z);
    r.top(Z);
    r.read(r.bwd, h);
    const int navail = (int)std::min<int64_t>(n, dev::NE_TOP);
    if (k >= 2 && h.topidx[0] == ind_best) { exit_code = NE_EXIT_HMAX_IS_BEST; break; }
    const int want = std::min<int>(navail, 2 + (int)ind_hist.size());
    auto seen = [&](long long i) { return std::find(ind_hist.begin(), ind_hist.end(), i) != ind_hist.end(); };
    if (seen(h.topidx[0]) && seen(h.topidx[1])) { exit_code = NE_EXIT_VISITED; break; }
    ind.clear();
    for (int q = 0; q < want; ++q) if (!seen(h.topidx[q])) ind.push_back(h.topidx[q]);
    for (int q = 0; q < want; ++q) if (seen(h.topidx[q])) ind.push_back(h.topidx[q]);
    r.zero(r.fwd);
    r.start(1, 0u, ind[0], ind[1]);
    for (int q = 0; q < 2; ++q) if (!seen(ind[q])) ind_hist.push_back(ind[q]);
    ++k;
  }
  HIPCHECK(hipGetLastError());
  finish();
}

}  // namespace

void normest_run(Ctx *c, Op &op, Op &adj, int p, double shift_re, double shift_im, int which, int64_t info[8], double *est) {
  const std::complex<double> sigma(shift_re, shift_im);
  c->use();
  try {
    dispatch_dtype(op.dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      // the 1-norm of M = (A - sigma I)^p takes A forward and A' backward; the infinity norm is the 1-norm of M'
      if (which == 1) normest_T<T>(c, op, adj, p, sigma, info, est);
      else normest_T<T>(c, adj, op, p, std::conj(sigma), info, est);
    });
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);      // (the work vectors go back to the context: nothing may still be writing them)
    throw;
  }
}

void normest_signs_host(int64_t n, int col, int64_t attempt, int8_t *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = (int8_t)normest_sign((uint64_t)i, (uint32_t)col, (uint32_t)attempt);
}

}  // namespace expv_mi
