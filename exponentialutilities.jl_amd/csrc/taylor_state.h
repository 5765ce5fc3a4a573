// taylor_state.h -- what every truncated-Taylor entry shares below the row sweep: the device-resident stage state, the arrival of
// a launch's workgroups, F's stopping test, the closing kernel, and THE ELEMENT STEP -- the one definition of the roundings of a
// term, used by the single, phiv, grid and block kernels, which is why their results agree bit for bit.  (The row sweep of the
// single-column families and the host-side launch setup: taylor_term.h.)  gfx950 only.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>

#include "kernel_common.h"

namespace expv_mi {
namespace dev {

// Stage state, 16 words of 8 bytes.  Inside a launch every word is touched by agent-scope atomics only (maxima, OR, ticket) or by
// lane 0 of the last workgroup to arrive, through L1-bypassing loads and stores; doubles travel as their bit patterns.
struct TaylorState {
  unsigned long long maxv, maxf;      // running maxima of |v_i| and |F_i| over the finite-or-infinite entries
  unsigned long long nanflags;        // bit 0 / 1: a NaN among v / F (the hardware maximum returns the other operand), bit 2: among the row sums
  unsigned long long ticket;
  unsigned long long stopped;         // the stage met its stopping test (or its v is zero): the rest of its term launches do nothing
  unsigned long long ended;           // a non-finite F ended the stage loop: every later launch does nothing
  unsigned long long c1;              // |v|_inf of the previous term
  unsigned long long fnorm;           // |F|_inf when the last stage closed
  unsigned long long apps, early;     // terms that entered F; stages stopped before m*
  unsigned long long nf_stage;        // 0, or 1 + the stage (from 0) whose F was not finite
  unsigned long long mu_re, mu_im;    // tr(A) / n
  unsigned long long rowmax;          // max_i ( |a_ii - mu| + sum_{j != i} |a_ij| )
  unsigned long long umax, wmax;      // phiv_taylor.hip: max |u_k[i]| and max_i sum_k |u_k[i]| over the columns k >= 1 of B
};
static_assert(sizeof(TaylorState) == 128, "TaylorState layout");

__device__ __forceinline__ unsigned long long ts_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ts_store(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ts_loadf(const unsigned long long *p) { return __longlong_as_double((long long)ts_load(p)); }
__device__ __forceinline__ void ts_storef(unsigned long long *p, double v) { ts_store(p, (unsigned long long)__double_as_longlong(v)); }

template <int OFF>
__device__ __forceinline__ double xor_max(double v) {      // max(v, v[lane ^ OFF]) in every lane; no NaN among the operands
  if constexpr (OFF >= 16) {
    double a = v, b = v;
    rows_swap<OFF>(a, b);
    return fmax(a, b);
  } else {
    return fmax(v, lane_xor<OFF>(v));
  }
}
__device__ __forceinline__ double wave_max(double v) {
  v = xor_max<32>(v);
  v = xor_max<16>(v);
  v = xor_max<8>(v);
  v = xor_max<4>(v);
  v = xor_max<2>(v);
  return xor_max<1>(v);
}

__device__ __forceinline__ double abs_T(double v) { return fabs(v); }
__device__ __forceinline__ double abs_T(float v) { return (double)fabsf(v); }
__device__ __forceinline__ double abs_T(cplx v) { return hypot(v.re, v.im); }
__device__ __forceinline__ double abs_T(cplx32 v) { return hypot((double)v.re, (double)v.im); }
// a maximum that keeps NaN out of the operands and remembers it in `bit` of nan
__device__ __forceinline__ void note_abs(double a, double &m, unsigned &nan, unsigned bit) {
  if (a != a) nan |= bit;
  else m = fmax(m, a);
}

__device__ __forceinline__ double taylor_qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- the element step: the roundings of one term, by definition ----
// Every operation below is either an explicit fused multiply-add or stands under `fp contract(off)`: the compiler has nothing to
// fuse or to leave unfused, so the same operands give the same bits in every kernel that calls these.
//   c a        real: the rounded product.  complex: re = fma(c.re, a.re, -(c.im a.im));  im = fma(c.re, a.im, c.im a.re) in
//              ComplexF64, fma(c.im, a.re, c.re a.im) in ComplexF32 (the pairing of the packed fp32 multiply-add).
//   F + c a    real: ONE fused multiply-add fma(c, a, F).  complex: the plain sum of F and the rounded c a, per component.
__device__ __forceinline__ double mul_as_single(double c, double a) {
#pragma clang fp contract(off)
  return c * a;
}
__device__ __forceinline__ float mul_as_single(float c, float a) {
#pragma clang fp contract(off)
  return c * a;
}
__device__ __forceinline__ cplx mul_as_single(cplx c, cplx a) {
#pragma clang fp contract(off)
  const double pr = c.im * a.im, pi = c.im * a.re;
  return make_cplx(fma(c.re, a.re, -pr), fma(c.re, a.im, pi));
}
__device__ __forceinline__ cplx32 mul_as_single(cplx32 c, cplx32 a) {
#pragma clang fp contract(off)
  const float pr = c.im * a.im, pi = c.re * a.im;
  return make_cplx32(fmaf(c.re, a.re, -pr), fmaf(c.im, a.re, pi));
}
// a + b as written, per component: never fused with the product that made b
template <class T>
__device__ __forceinline__ T add_as_written(T a, T b) {
#pragma clang fp contract(off)
  if constexpr (ST<T>::is_complex) {
    a.re = a.re + b.re;
    a.im = a.im + b.im;
    return a;
  } else {
    return a + b;
  }
}
// F + c a, given y = mul_as_single(c, a)
template <class T>
__device__ __forceinline__ T term_sum(T f, T c, T a, T y) {
  if constexpr (ST<T>::is_complex) {
    return add_as_written(f, y);
  } else {
    ST<T>::fma_(f, c, a);
    return f;
  }
}
// One element of a term in two halves: v = acc - mu x_i (acc = (A x)_i) and cv = c v, the next v_i ...
template <class T>
__device__ __forceinline__ void taylor_product(T acc, T mu, T xi, T c, T &v, T &cv) {
  v = acc;
  ST<T>::nfma(v, mu, xi);
  cv = mul_as_single(c, v);
}
// ... and fn = F_i + c v.  (A family that adds to cv before it enters F takes the first half and owns the sum: phiv_taylor.hip.)
template <class T>
__device__ __forceinline__ void taylor_step(T acc, T mu, T xi, T c, T f, T &cv, T &fn) {
  T v;
  taylor_product(acc, mu, xi, c, v, cv);
  fn = term_sum<T>(f, c, v, cv);
}

// ---- one launch of the series: arrival, the stopping test, the closing kernel ----

// Every thread of every workgroup of a launch: this workgroup's maxima into the state, then one ticket.  True in the workgroup that
// arrives last, whose lane 0 then owns the state (everything the others added was performed before their tickets).
__device__ __forceinline__ bool taylor_arrive(TaylorState *st, double mv, double mf, unsigned nan) {
  __shared__ double mv_s[BLOCK / 64], mf_s[BLOCK / 64];
  __shared__ unsigned nan_s[BLOCK / 64];
  __shared__ int last_s;
  mv = wave_max(mv);
  mf = wave_max(mf);
  nan = (__any((int)(nan & 1u)) ? 1u : 0u) | (__any((int)(nan & 2u)) ? 2u : 0u) | (__any((int)(nan & 4u)) ? 4u : 0u);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { mv_s[wave] = mv; mf_s[wave] = mf; nan_s[wave] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) { mv = fmax(mv, mv_s[w]); mf = fmax(mf, mf_s[w]); nan |= nan_s[w]; }
    if (mv > 0.0) atomicMax(&st->maxv, (unsigned long long)__double_as_longlong(mv));
    if (mf > 0.0) atomicMax(&st->maxf, (unsigned long long)__double_as_longlong(mf));
    if (nan) atomicOr(&st->nanflags, (unsigned long long)nan);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __hip_atomic_fetch_add(&st->ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = (t == (unsigned long long)gridDim.x - 1ull);
  }
  __syncthreads();
  return last_s != 0;
}
__device__ __forceinline__ void taylor_rearm(TaylorState *st) {
  ts_store(&st->maxv, 0ull);
  ts_store(&st->maxf, 0ull);
  ts_store(&st->nanflags, 0ull);
  ts_store(&st->ticket, 0ull);
}
// lane 0 of the last workgroup of a term launch.  `nan` is the state's nanflags word, read ONCE per test: every access below is a
// round trip to device memory on the critical path of the launch, so the loads of a test are issued together, ahead of its stores.
__device__ __forceinline__ double taylor_vmax(const TaylorState *st, unsigned long long nan) {      // |v_j|_inf (NaN when v held one)
  return (nan & 1ull) ? taylor_qnan() : ts_loadf(&st->maxv);
}
__device__ __forceinline__ double taylor_fnorm(const TaylorState *st, unsigned long long nan) {     // |F|_inf (NaN when F held one)
  return (nan & 2ull) ? taylor_qnan() : ts_loadf(&st->maxf);
}
// F's test of the reference's loop (:153-155): c1 = |v_{j-1}|_inf, c2 = |v_j|_inf, fn = |F|_inf
__device__ __forceinline__ void taylor_f_test(TaylorState *st, double c1, double c2, double fn, double tol, int j, int m) {
  if (c1 + c2 <= tol * fn) {
    ts_store(&st->stopped, 1ull);
    if (j < m) ts_store(&st->early, ts_load(&st->early) + 1ull);
  } else {
    ts_storef(&st->c1, c2);
  }
}
// The whole test of a single-column term.  tail: a floor under |v|_inf (the part of the term that lives outside the n rows,
// phiv_taylor.hip; 0 for exp(tA)b, where max(x, 0) = x for the non-negative maximum)
__device__ __forceinline__ void taylor_term_test(TaylorState *st, double tol, int j, int m, double tail) {
  const unsigned long long nan = ts_load(&st->nanflags);
  const double c2 = (nan & 1ull) ? taylor_qnan() : fmax(ts_loadf(&st->maxv), tail);
  const double fn = taylor_fnorm(st, nan);
  const double c1 = ts_loadf(&st->c1);
  ts_store(&st->apps, ts_load(&st->apps) + 1ull);
  taylor_f_test(st, c1, c2, fn, tol, j, m);
  taylor_rearm(st);
}
__device__ __forceinline__ bool taylor_skip(const TaylorState *st) {
  return (ts_load(&st->stopped) | ts_load(&st->ended)) != 0ull;
}

// Closes a stage (:157-159): F = eta src (scale == 0: F = src as it is), v = F, c1 = |F|_inf, the finite test, and the state of the
// next stage.  The first launch of a call is this kernel with src = b, scale = 0 and stage = -1 (no finite test: the reference
// looks at F only after a stage).  tail: the floor under c1 of the stage that follows (taylor_term_test; 0 for exp(tA)b).
template <class T>
__global__ __launch_bounds__(BLOCK) void k_taylor_close(const T *src, T *F, T *v, int64_t n, T eta, int scale, int stage, int more,
                                                        double tail, TaylorState *st) {
  if (ts_load(&st->ended) != 0ull) return;
  constexpr int N = Pack<T>::N;
  const bool als = is_al16(src), alf = is_al16(F), alv = is_al16(v);
  double mf = 0.0;
  unsigned nan = 0u;
  for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * N; i < n; i += (int64_t)gridDim.x * BLOCK * N) {
    Pack<T> f = ld_pack_user(src, i, n, als);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (scale) f.v[k] = mul_as_single(eta, f.v[k]);
      if (i + k < n) note_abs(abs_T(f.v[k]), mf, nan, 2u);
    }
    if (scale || src != F) st_pack_user(F, i, n, alf, f);
    st_pack_user(v, i, n, alv, f);
  }
  if (taylor_arrive(st, 0.0, mf, nan) && threadIdx.x == 0) {
    const double fn = (ts_load(&st->nanflags) & 2ull) ? taylor_qnan() : ts_loadf(&st->maxf);
    ts_storef(&st->c1, fn != fn ? fn : fmax(fn, tail));
    ts_storef(&st->fnorm, fn);
    const bool finite = fn < __longlong_as_double(0x7ff0000000000000ll);
    if (stage >= 0 && !finite) {
      ts_store(&st->ended, 1ull);
      ts_store(&st->nf_stage, (unsigned long long)stage + 1ull);
    }
    // a zero vector stays zero: the stage that follows applies nothing (b = 0 costs no operator application)
    const bool zero = fn == 0.0 && tail == 0.0;
    ts_store(&st->stopped, zero ? 1ull : 0ull);
    if (zero && more) ts_store(&st->early, ts_load(&st->early) + 1ull);
    taylor_rearm(st);
  }
}

// workgroups for `items` rows (or slices) at `per_block` each
static int taylor_grid(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, MAX_GRID));
}

}  // namespace dev

static inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
static inline double f64_of(unsigned long long u) { double d; std::memcpy(&d, &u, 8); return d; }

// The stage factor exp(mu t / s) in double.  The complex product is spelled out: written as mu * t the host compiler fuses one
// product of each component into a multiply-add and picks WHICH ONE from the code around, so that two callers disagree in the last
// bit when mu and t are both complex -- and with them every bit-for-bit promise between the single, block and grid calls.  With
// the product written out nothing is left to choose.  (For a real mu or a real t every form rounds alike; for a complex mu with a
// complex t the factor of expv_taylor and expv_taylor_block may differ in its last bit from what they computed before this helper.)
static inline std::complex<double> taylor_stage_factor(std::complex<double> mu, std::complex<double> t, int64_t ns) {
  const double pr = mu.imag() * t.imag(), pi = mu.imag() * t.real();
  const double re = std::fma(mu.real(), t.real(), -pr), im = std::fma(mu.real(), t.imag(), pi);
  return std::exp(std::complex<double>(re / (double)ns, im / (double)ns));
}

// a host scalar rounded to the element type the kernels take it in
template <class T> static inline T taylor_scalar(std::complex<double> z) {
  if constexpr (ST<T>::is_complex) { T r; r.re = (typename ST<T>::real_t)z.real(); r.im = (typename ST<T>::real_t)z.imag(); return r; }
  else return (T)z.real();
}

}  // namespace expv_mi
