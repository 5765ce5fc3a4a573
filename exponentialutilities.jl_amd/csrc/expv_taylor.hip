// expv_taylor.hip -- exp(tA)b by the truncated Taylor series of Al-Mohy & Higham (SIAM J. Sci. Comput. 33, 2011): no Krylov basis,
// no inner product, three work vectors.
//
//   ext/ExponentialUtilitiesStaticArraysExt.jl:124-163 of the reference (the iteration), :76-103 (m*, s), :10-73 (theta tables)
//
//   mu = tr(A) / n, alpha = |t| ||A - mu I||_inf, (m*, s) = argmin m ceil(alpha / theta_m);  F = v = b;  s stages of
//       c1 = |v|_inf;  for j = 1 .. m*:  v <- (t / s)(A - mu I) v / j,  F += v,  c2 = |v|_inf,  stop when c1 + c2 <= tol |F|_inf, c1 = c2
//       F *= exp(mu t / s),  v = F,  leave when F is not finite
//
// The reference takes opnorm(A, 1) and stops at N <= 50 because it has no norm estimator; here the norm is the EXACT infinity norm,
// one pass over the rows the operator already stores (a row maximum is order-independent, and the truncation analysis holds in any
// subordinate norm).  The stopping rule lives on the device: every term kernel folds its workgroups' maxima of |v_i| and |F_i| into
// the stage state with integer atomic maxima (non-negative doubles order like their bit patterns: the result does not depend on
// arrival order), the last workgroup to arrive applies the test and publishes `stopped`, and the remaining term launches of the
// stage return at once.  The host enqueues s (m* + 1) launches and reads nothing in between.
//
// Traffic per term: fused kernel (SELL slots without overflow, or the general diagonal form): the operator + x gather, x_i, F read,
// y and F written -- the operator plus four vector streams.  Everything else: mul! (operator, x, y) + one update pass over x, y, F.
//
// This file holds the plan (mu, alpha, m*, s), the reference's whole parameter search behind power norms (taylor_params_power; the norms
// come from op_normest.hip) and the host loop of the single call.  The term kernel k_taylor_term<T, FUSED>, its row
// sweep and the launch setup shared with the phiv and grid entries are in taylor_term.h; the stage state, the closing kernel and the
// element step that fixes the roundings of a term are in taylor_state.h.
#include <cmath>
#include <complex>
#include <limits>

#include "engine.h"
#include "kernel_common.h"
#include "taylor_state.h"
#include "taylor_term.h"
#include "taylor_theta.h"

namespace expv_mi {
namespace dev {

// mu = tr(A) / n and ||A - mu I||_inf of a stored operator, in two launches of one kernel over the arrays the operator keeps:
// mode 0 sums the diagonal (per-workgroup partials, finished by the last workgroup in index order: the same bits every run) and
// leaves mu in the state; mode 1 takes max_i (|a_ii - mu| + sum_{j != i} |a_ij|), |mu| for a row without a stored diagonal entry.
// rp == nullptr: the dense column-major block `val` with leading dimension lda.  Repeated entries of a CSR row count one by one
// off the diagonal (an upper bound of the summed entry) and are summed on it.
template <class T>
__global__ __launch_bounds__(BLOCK) void k_taylor_shift_norm(int mode, int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                            const T *__restrict__ val, int64_t lda, double *part, TaylorState *st) {
  __shared__ double red_s[BLOCK / 64];
  const cplx mu = make_cplx(mode ? ts_loadf(&st->mu_re) : 0.0, mode ? ts_loadf(&st->mu_im) : 0.0);
  double tr_re = 0.0, tr_im = 0.0, best = 0.0;
  unsigned nan = 0u;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * BLOCK) {
    double d_re = 0.0, d_im = 0.0, off = 0.0;
    auto take = [&](T v, bool diag) {
      if (diag) {
        if constexpr (ST<T>::is_complex) { d_re += (double)v.re; d_im += (double)v.im; }
        else d_re += (double)v;
      } else if (mode) {
        off += abs_T(v);
      }
    };
    if (rp) {
      for (int32_t k = rp[r]; k < rp[r + 1]; ++k) take(val[k], ci[k] == (int32_t)r);
    } else if (mode) {
      for (int64_t j = 0; j < n; ++j) take(val[r + j * lda], j == r);
    } else {
      take(val[r + r * lda], true);
    }
    tr_re += d_re;
    tr_im += d_im;
    if (mode) note_abs(off + hypot(d_re - mu.re, d_im - mu.im), best, nan, 4u);
  }
  if (mode) {
    if (taylor_arrive(st, 0.0, best, nan) && threadIdx.x == 0) {
      ts_store(&st->rowmax, ts_load(&st->maxf));
      const unsigned long long nf = ts_load(&st->nanflags);
      taylor_rearm(st);
      ts_store(&st->nanflags, nf & 4ull);      // (read by the host, cleared by the first closing launch)
    }
    return;
  }
  const double b_re = block_sum(tr_re, red_s);
  __syncthreads();
  const double b_im = block_sum(tr_im, red_s);
  if (threadIdx.x == 0) {
    publish_f64(part + blockIdx.x, b_re);
    publish_f64(part + MAX_GRID + blockIdx.x, b_im);
  }
  if (!taylor_arrive(st, 0.0, 0.0, 0u)) return;
  double s_re = 0.0, s_im = 0.0;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += BLOCK) {
    s_re += consume_f64(part + b);
    s_im += consume_f64(part + MAX_GRID + b);
  }
  __syncthreads();
  s_re = block_sum(s_re, red_s);
  __syncthreads();
  s_im = block_sum(s_im, red_s);
  if (threadIdx.x == 0) {
    ts_storef(&st->mu_re, s_re / (double)n);
    ts_storef(&st->mu_im, s_im / (double)n);
    taylor_rearm(st);
  }
}

}  // namespace dev

// ------------------------------------------------------------------------------------------
// parameters                                     ExponentialUtilitiesStaticArraysExt.jl:76-103
// ------------------------------------------------------------------------------------------
static const double *taylor_table(int precision) {
  if (precision == 0) return TAYLOR_THETA64;
  if (precision == 1) return TAYLOR_THETA32;
  fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: precision must be 0 (working precision) or 1 (2^-24)");
}
double taylor_theta(int precision, int m) {
  const double *th = taylor_table(precision);
  if (m < 1 || m > TAYLOR_M_MAX) fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: theta_m is tabulated for m = 1 .. 55");
  return th[m - 1];
}
void taylor_params(int precision, double alpha, int *m_out, int64_t *s_out) {
  const double *th = taylor_table(precision);
  if (!(alpha >= 0.0) || !std::isfinite(alpha))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: alpha = |t| opnorm(A - mu I, Inf) = " + std::to_string(alpha) + " is not a finite non-negative number");
  if (alpha == 0.0) { *m_out = 0; *s_out = 1; return; }
  int best_m = 0;
  double best_s = 0.0;
  unsigned __int128 best_cost = 0;
  for (int m = 1; m <= TAYLOR_M_MAX; ++m) {
    const double sd = std::ceil(alpha / th[m - 1]);
    if (!(sd < 0x1p100)) continue;      // (not a candidate: its cost is far beyond every 64-bit count)
    const unsigned __int128 cost = (unsigned __int128)sd * (unsigned)m;
    if (best_m == 0 || cost < best_cost) { best_m = m; best_s = sd; best_cost = cost; }      // first minimum on ties
  }
  if (best_m == 0 || !(best_s < 0x1p62))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: alpha = " + std::to_string(alpha) + " needs more stages than a 64-bit count holds");
  *m_out = best_m;
  *s_out = (int64_t)best_s;
}

// The whole search (:99-121), given alpha_1 and d[i] = ||B^(i+2)||^(1/(i+2)), i = 0 .. 7 (d_2 .. d_9, |t| folded in).  Below the cheap
// threshold 4 theta_55 P (P + 3) / 55, P = 8, the first branch; otherwise for p = 2 .. 8 alpha_p = max(d_p, d_{p+1}) and the first
// minimum of m ceil(alpha_p / theta_m) over p (p - 1) - 1 <= m <= 55; the overall minimum by (cost, m), the first p that reaches it;
// s = max(cost / m, 1).  A candidate whose stage count is beyond every 64-bit count is skipped, as in taylor_params.
double taylor_power_threshold(int precision) {
  return 4.0 * taylor_table(precision)[TAYLOR_M_MAX - 1] * 8.0 * 11.0 / 55.0;
}
void taylor_params_power(int precision, double alpha1, const double d[8], int *m_out, int64_t *s_out, int *p_used) {
  const double *th = taylor_table(precision);
  if (!(alpha1 >= 0.0) || !std::isfinite(alpha1))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: alpha = |t| opnorm(A - mu I, Inf) = " + std::to_string(alpha1) + " is not a finite non-negative number");
  *p_used = 0;
  if (alpha1 == 0.0) { *m_out = 0; *s_out = 1; return; }
  if (alpha1 <= taylor_power_threshold(precision)) { taylor_params(precision, alpha1, m_out, s_out); return; }
  for (int i = 0; i < 8; ++i)
    if (!(d[i] >= 0.0) || !std::isfinite(d[i]))
      fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: d_" + std::to_string(i + 2) + " = " + std::to_string(d[i]) + " is not a finite non-negative number");
  bool have = false;
  unsigned __int128 best_cost = 0;
  int best_m = 1, best_p = 0;
  for (int p = 2; p <= 8; ++p) {
    const double ap = std::max(d[p - 2], d[p - 1]);
    bool have_p = false;
    unsigned __int128 cost_p = 0;
    int m_p = 0;
    for (int m = p * (p - 1) - 1; m <= TAYLOR_M_MAX; ++m) {
      const double sd = std::ceil(ap / th[m - 1]);
      if (!(sd < 0x1p100)) continue;
      const unsigned __int128 cost = (unsigned __int128)sd * (unsigned)m;
      if (!have_p || cost < cost_p) { have_p = true; cost_p = cost; m_p = m; }
    }
    if (have_p && (!have || cost_p < best_cost || (cost_p == best_cost && m_p < best_m))) { have = true; best_cost = cost_p; best_m = m_p; best_p = p; }
  }
  const unsigned __int128 sq = have ? best_cost / (unsigned)best_m : 0;
  if (!have || !(sq < ((unsigned __int128)1 << 62)))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: alpha = " + std::to_string(alpha1) + " needs more stages than a 64-bit count holds");
  *m_out = best_m;
  *s_out = std::max<int64_t>((int64_t)sq, 1);
  *p_used = best_p;
}

// ------------------------------------------------------------------------------------------
// the call
// ------------------------------------------------------------------------------------------
size_t taylor_head_bytes() { return sizeof(dev::TaylorState) + sizeof(double) * 2 * dev::MAX_GRID; }

// (m*, s) and tol for tc.alpha, and the max_matvecs refusal
void taylor_choose(const Op &op, int precision, int64_t max_matvecs, TaylorCall &tc) {
  const int table = (precision == 1 || dtype_is_32bit(op.dtype)) ? 1 : 0;      // precision 0: the working precision of the operator's real type
  taylor_params(table, tc.alpha, &tc.m, &tc.s);
  const int m = tc.m;
  const int64_t ns = tc.s;
  if (max_matvecs > 0 && (unsigned __int128)ns * (unsigned)m > (unsigned __int128)max_matvecs)
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: alpha = " + std::to_string(tc.alpha) + " needs m* = " + std::to_string(m) + " terms in each of s = " +
                                     std::to_string(ns) + " stages, more than max_matvecs = " + std::to_string(max_matvecs));
  tc.tol = table == 1 ? 0x1p-24 : 0x1p-53;
}

// What depends on A and t alone: mu, alpha (two launches and the one blocking read of a stored operator) and (m*, s).  `head`:
// taylor_head_bytes() of device memory, zeroed here; its state block is ready for the first closing launch of a call afterwards.
template <class T>
static void taylor_shift_plan_T(Ctx *c, Op &op, std::complex<double> t, int precision, int64_t max_matvecs, double opnorm, void *head,
                                TaylorCall &tc) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  dev::TaylorState *st = reinterpret_cast<dev::TaylorState *>(head);
  double *part = reinterpret_cast<double *>(static_cast<char *>(head) + sizeof(dev::TaylorState));
  HIPCHECK(hipMemsetAsync(st, 0, sizeof(dev::TaylorState), s));

  // shift and norm
  std::complex<double> mu(0.0, 0.0);
  double anorm = opnorm;
  if (op.kind != OP_CALLBACK) {
    const bool dense = op.kind == OP_DENSE;
    if (!dense && !(op.rowptr.p && (op.nnz == 0 || (op.col.p && op.val.p)))) fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: sparse operator without its CSR arrays");
    const int g = dev::taylor_grid(n, dev::BLOCK);
    for (int mode = 0; mode < 2; ++mode) {
      ProfScope ps(c, EXPV_MI_K_LINCOMB);
      hipLaunchKernelGGL(dev::k_taylor_shift_norm<T>, dim3(g), dim3(dev::BLOCK), 0, s, mode, n, dense ? nullptr : op.rowptr.as<int32_t>(),
                         dense ? nullptr : op.col.as<int32_t>(), dense ? reinterpret_cast<const T *>(op.dense_ptr) : op.val.as<T>(),
                         dense ? op.lda : (int64_t)0, part, st);
    }
    dev::TaylorState h;
    HIPCHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    ++tc.reads;
    mu = std::complex<double>(f64_of(h.mu_re), f64_of(h.mu_im));
    anorm = (h.nanflags & 4ull) ? std::numeric_limits<double>::quiet_NaN() : f64_of(h.rowmax);
  }
  tc.mu_re = mu.real();
  tc.mu_im = mu.imag();
  tc.alpha = std::abs(t) * anorm;
  if (std::abs(t) == 0.0 || anorm == 0.0) tc.alpha = 0.0;      // (0 * Inf: t = 0 returns b whatever A holds)
  taylor_choose(op, precision, max_matvecs, tc);
}

// Every launch of one vector's series behind a plan: F = v = b, then s stages.  `st` is a zeroed state block (or the one the plan
// left); v0, v1 and F hold n elements each; b may be F itself.
template <class T>
static void taylor_run_T(Ctx *c, Op &op, std::complex<double> t, const void *b_dev, void *state, void *v0, void *v1, void *Fv, TaylorCall &tc) {
  T *V[2] = {reinterpret_cast<T *>(v0), reinterpret_cast<T *>(v1)};
  const int64_t ns = tc.s;
  const TaylorLaunch<T> L(c, op, tc, reinterpret_cast<T *>(Fv), reinterpret_cast<dev::TaylorState *>(state));
  dev::TaylorTermArgs<T> a = L.args();
  const std::complex<double> eta = taylor_stage_factor(std::complex<double>(tc.mu_re, tc.mu_im), t, ns);
  int p = 0;
  L.close(reinterpret_cast<const T *>(b_dev), V[0], eta, -1, 0.0);
  for (int64_t stage = 0; stage < ns; ++stage) {
    for (int j = 1; j <= tc.m; ++j) {
      a.x = V[p]; a.y = V[1 - p]; a.j = j;
      a.c = taylor_scalar<T>(t / (double)ns / (double)j);
      L.term(a, a.x, a.y, [](auto fused) { return dev::k_taylor_term<T, decltype(fused)::value>; });
      p ^= 1;
    }
    L.close(L.F, V[p], eta, stage, 0.0);
  }
  HIPCHECK(hipGetLastError());
}

bool taylor_fused(const Op &op) { return op.kind == OP_CSR && op.sell_ok && op.ovf_nseg == 0 && !op.cbf; }

void taylor_check(const Op &op, double t_im, int precision, double opnorm) {
  (void)taylor_table(precision);
  if (t_im != 0.0 && !dtype_is_complex(op.dtype))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: a complex t needs a complex operator (a real operator with a complex result is not computed)");
  if (op.kind == OP_CALLBACK && !(opnorm > 0.0 && std::isfinite(opnorm)))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: a matrix-free operator needs opnorm > 0, a bound on opnorm(A, Inf)");
}
void taylor_shift_plan(Ctx *c, Op &op, double t_re, double t_im, int precision, int64_t max_matvecs, double opnorm, void *head, TaylorCall &tc) {
  taylor_check(op, t_im, precision, opnorm);
  dispatch_dtype(op.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    taylor_shift_plan_T<T>(c, op, std::complex<double>(t_re, t_im), precision, max_matvecs, opnorm, head, tc);
  });
}
// The plan of a REAL operator for a complex t (expv_taylor_realop.hip): the checks of taylor_check that do not concern t, then the
// same kernels in the operator's real type -- mu is real, alpha = |t| ||A - mu I||_inf.
void taylor_shift_plan_realop(Ctx *c, Op &op, double t_re, double t_im, int precision, int64_t max_matvecs, double opnorm, void *head,
                              TaylorCall &tc) {
  taylor_check(op, 0.0, precision, opnorm);
  if (op.dtype == EXPV_MI_F32) taylor_shift_plan_T<float>(c, op, std::complex<double>(t_re, t_im), precision, max_matvecs, opnorm, head, tc);
  else taylor_shift_plan_T<double>(c, op, std::complex<double>(t_re, t_im), precision, max_matvecs, opnorm, head, tc);
}
void taylor_run(Ctx *c, Op &op, double t_re, double t_im, const void *b_dev, void *state, void *v0, void *v1, void *F, TaylorCall &tc) {
  dispatch_dtype(op.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    taylor_run_T<T>(c, op, std::complex<double>(t_re, t_im), b_dev, state, v0, v1, F, tc);
  });
}

void taylor_enqueue(Ctx *c, Op &op, double t_re, double t_im, const void *b_dev, int precision, int64_t max_matvecs, double opnorm,
                    TaylorCall &tc) {
  c->use();
  try {
    const size_t vbytes = up16((size_t)op.n * dtype_size(op.dtype)) + 16, head = taylor_head_bytes();
    tc.work.take_from(c, head + 3 * vbytes);
    char *base = tc.work.as<char>();
    tc.state = base;
    tc.F = base + head + 2 * vbytes;
    taylor_shift_plan(c, op, t_re, t_im, precision, max_matvecs, opnorm, base, tc);
    taylor_run(c, op, t_re, t_im, b_dev, base, base + head, base + head + vbytes, tc.F, tc);
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);      // (the work vectors go back to the context: nothing may still be writing them)
    throw;
  }
}

// ||A - sigma I||_inf of a stored operator, exactly: the norm pass of the plan with sigma in the place of mu (one blocking read)
double taylor_rownorm(Ctx *c, Op &op, double sigma_re, double sigma_im) {
  c->use();
  DevBuf head;
  head.take_from(c, taylor_head_bytes());
  dev::TaylorState h;
  try {
    dispatch_dtype(op.dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipStream_t s = c->stream;
      dev::TaylorState *st = head.as<dev::TaylorState>();
      std::memset(&h, 0, sizeof(h));
      std::memcpy(&h.mu_re, &sigma_re, 8);
      std::memcpy(&h.mu_im, &sigma_im, 8);
      HIPCHECK(hipMemcpyAsync(st, &h, sizeof(h), hipMemcpyHostToDevice, s));
      const bool dense = op.kind == OP_DENSE;
      if (!dense && !(op.rowptr.p && (op.nnz == 0 || (op.col.p && op.val.p)))) fail(EXPV_MI_ARGUMENT_ERROR, "op_norm_power: sparse operator without its CSR arrays");
      {
        ProfScope ps(c, EXPV_MI_K_LINCOMB);
        hipLaunchKernelGGL(dev::k_taylor_shift_norm<T>, dim3(dev::taylor_grid(op.n, dev::BLOCK)), dim3(dev::BLOCK), 0, s, 1, op.n,
                           dense ? nullptr : op.rowptr.as<int32_t>(), dense ? nullptr : op.col.as<int32_t>(),
                           dense ? reinterpret_cast<const T *>(op.dense_ptr) : op.val.as<T>(), dense ? op.lda : (int64_t)0,
                           reinterpret_cast<double *>(head.as<char>() + sizeof(dev::TaylorState)), st);
      }
      HIPCHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
    });
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    throw;
  }
  return (h.nanflags & 4ull) ? std::numeric_limits<double>::quiet_NaN() : f64_of(h.rowmax);
}

// expv_taylor with the whole parameter search: the plan of taylor_enqueue, then -- above the cheap threshold -- d_2 .. d_9 of
// B = A - mu I from the norm estimator and (m*, s) from taylor_params_power, then the unchanged series.  pinfo: p_used, the
// estimator's panel applications, its blocking reads; d[8]: d_2 .. d_9 (zeros when nothing was estimated).
void taylor_power_enqueue(Ctx *c, Op &op, const std::function<Op &()> &get_adj, double t_re, double t_im, const void *b_dev, int precision, int64_t max_matvecs,
                          TaylorCall &tc, int64_t pinfo[3], double d[8]) {
  c->use();
  try {
    const size_t vbytes = up16((size_t)op.n * dtype_size(op.dtype)) + 16, head = taylor_head_bytes();
    tc.work.take_from(c, head + 3 * vbytes);
    char *base = tc.work.as<char>();
    tc.state = base;
    tc.F = base + head + 2 * vbytes;
    taylor_shift_plan(c, op, t_re, t_im, precision, 0, 0.0, base, tc);      // (the refusal waits for the refined parameters)
    const int table = (precision == 1 || dtype_is_32bit(op.dtype)) ? 1 : 0;
    if (tc.alpha != 0.0 && tc.alpha > taylor_power_threshold(table)) {
      const double at = std::hypot(t_re, t_im);
      Op &adj = get_adj();
      for (int p = 2; p <= 9; ++p) {
        int64_t ninfo[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double est = 0.0;
        normest_run(c, op, adj, p, tc.mu_re, tc.mu_im, 0, ninfo, &est);
        d[p - 2] = at * std::pow(est, 1.0 / (double)p);
        pinfo[1] += ninfo[1];
        pinfo[2] += ninfo[2];
      }
      int p_used = 0;
      taylor_params_power(table, tc.alpha, d, &tc.m, &tc.s, &p_used);
      pinfo[0] = p_used;
    }
    if (max_matvecs > 0 && (unsigned __int128)tc.s * (unsigned)tc.m > (unsigned __int128)max_matvecs)
      fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: alpha = " + std::to_string(tc.alpha) + " needs m* = " + std::to_string(tc.m) + " terms in each of s = " +
                                       std::to_string(tc.s) + " stages, more than max_matvecs = " + std::to_string(max_matvecs));
    taylor_run(c, op, t_re, t_im, b_dev, base, base + head, base + head + vbytes, tc.F, tc);
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    throw;
  }
}

void taylor_collect(Ctx *c, TaylorCall &tc, int64_t info[8], double dinfo[4]) {
  dev::TaylorState h;
  HIPCHECK(hipMemcpyAsync(&h, tc.state, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  ++tc.reads;
  taylor_fill_info(tc, h, info, dinfo);
}

}  // namespace expv_mi
