// taylor_state.h -- the device-resident stage state of the truncated-Taylor exp(tA)b and the helpers its kernels share
// (expv_taylor.hip: one vector; expv_taylor_block.hip: a block of columns).  gfx950 only.
#pragma once
#include <complex>

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
  unsigned long long spare[2];
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

}  // namespace dev

// a host scalar rounded to the element type the kernels take it in
template <class T> static inline T taylor_scalar(std::complex<double> z) {
  if constexpr (ST<T>::is_complex) { T r; r.re = (typename ST<T>::real_t)z.real(); r.im = (typename ST<T>::real_t)z.imag(); return r; }
  else return (T)z.real();
}

}  // namespace expv_mi
