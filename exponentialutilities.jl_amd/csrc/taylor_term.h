// taylor_term.h -- one term of the truncated Taylor series for the single-column families (expv_taylor.hip: exp(tA)b;
// expv_taylor_grid.hip: the same with a panel of interior outputs), and the host side of launching it, which phiv_taylor.hip uses too
// (its term kernel keeps loops of its own, for the reason given there).  The row loop is written ONCE (taylor_sweep): load x_i and F, take (A x)_i from the operator (FUSED: SELL slots
// without overflow, or the general diagonal form) or from y as mul! left it, the element step of taylor_state.h, maxima over the
// rows below n, store.  What the grid adds is a small policy object the sweep calls.  The block kernel
// (expv_taylor_block.hip) has its own loop over [row][P] vectors and shares the element step, the operator view and the launch
// bookkeeping.  gfx950 only.
#pragma once
#include "engine.h"
#include "kernel_common.h"
#include "sparse_rows.h"
#include "taylor_state.h"

namespace expv_mi {
namespace dev {

template <class T>
struct TaylorOpView {                             // the operator as a fused term kernel reads it
  SellView<T> A;                                  // SELL slots (ndiag == 0) ...
  const T *dia_val; int64_t dia_ld; int ndiag; const int32_t *dia_off;      // ... or the general diagonal form
};

template <class T>
struct TaylorTermArgs {
  TaylorOpView<T> op;                             // (FUSED kernels only)
  const T *x;                                     // v of the previous term
  T *y;                                           // FUSED: out.  otherwise: in (A x as mul! left it) and out
  T *F;
  int64_t n;
  T c, mu;                                        // (t / s) / j and tr(A) / n
  double tol;
  int j, m;
  TaylorState *st;
};

// The policy of a family without extras (exp(tA)b), and the interface of every policy:
//   fstop        F has met its own test while v goes on: F is written back as it is and gives no maximum
//   rows(i, ..)  behind the stores of y and F: further work on the pack's rows
struct TermPlain {
  static constexpr bool fstop = false;
  template <class T> __device__ __forceinline__ void rows(int64_t, const Pack<T> &, const Pack<T> &) {}
};

// y_i = c ((A x)_i - mu x_i), F_i += y_i, and this thread's maxima of |y_i| and |F_i|: one term of the series
// in one pass.  Both forms give thread (block, tid) the packs (block BLOCK + tid + k gridDim BLOCK) N; the fused one walks them by
// slice, whole slices only, so that every lane of a wave is there for the slots of its slice.
template <class T, bool FUSED, class X>
__device__ __forceinline__ void taylor_sweep(const TaylorTermArgs<T> &a, X &x, double &mv, double &mf, unsigned &nan) {
  constexpr int N = Pack<T>::N;
  constexpr int SH = 64 * N;
  const bool alx = is_al16(a.x), aly = is_al16(a.y), alf = is_al16(a.F);
  auto pack = [&](int64_t i, int64_t slice, int lane) {
    const Pack<T> xi = ld_pack_user(a.x, i, a.n, alx);      // independent of the operator: in flight with its slots
    Pack<T> acc;
    if constexpr (!FUSED) acc = ld_pack_user(a.y, i, a.n, aly);
    Pack<T> f = ld_pack_user(a.F, i, a.n, alf);
    if constexpr (FUSED) {
      if (a.op.ndiag > 0) dia_rows<T>(a.op.dia_val, a.op.dia_ld, a.op.ndiag, a.op.dia_off, i, a.n, a.x, acc.v);
      else sell_rows<T>(a.op.A, slice, lane, a.x, acc.v);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      T cv, fn;
      taylor_step(acc.v[k], a.mu, xi.v[k], a.c, f.v[k], cv, fn);
      acc.v[k] = cv;
      if (!x.fstop) f.v[k] = fn;
      if (i + k < a.n) {      // (rows of the last pack beyond n hold what the padding slots gave: not part of the vector)
        note_abs(abs_T(cv), mv, nan, 1u);
        if (!x.fstop) note_abs(abs_T(fn), mf, nan, 2u);
      }
    }
    st_pack_user(a.y, i, a.n, aly, acc);
    st_pack_user(a.F, i, a.n, alf, f);
    x.rows(i, xi, acc);
  };
  if constexpr (FUSED) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nsl = (a.n + SH - 1) / SH;
    for (int64_t slice = (int64_t)blockIdx.x * (BLOCK / 64) + wave; slice < nsl; slice += (int64_t)gridDim.x * (BLOCK / 64))
      pack(slice * SH + (int64_t)lane * N, slice, lane);
  } else {
    for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * N; i < a.n; i += (int64_t)gridDim.x * BLOCK * N) pack(i, 0, 0);
  }
}

// exp(tA)b: the sweep, the arrival, the test
template <class T, bool FUSED>
__global__ __launch_bounds__(BLOCK) void k_taylor_term(TaylorTermArgs<T> a) {
  if (taylor_skip(a.st)) return;
  double mv = 0.0, mf = 0.0;
  unsigned nan = 0u;
  TermPlain x;
  taylor_sweep<T, FUSED>(a, x, mv, mf, nan);
  if (taylor_arrive(a.st, mv, mf, nan) && threadIdx.x == 0) taylor_term_test(a.st, a.tol, a.j, a.m, 0.0);
}

}  // namespace dev

// ---- the host side of a term launch ----

// the operator of a fused call as its term kernels read it
template <class T>
dev::TaylorOpView<T> taylor_op_view(const Ctx *c, const Op &op) {
  dev::TaylorOpView<T> v{};
  v.A = dev::SellView<T>{op.sell_off.as<int64_t>(), op.sell_col.as<int32_t>(), op.sell_val.as<T>(), op.nslices};
  if (op.gndiag > 0 && c->opt.dia) {
    v.dia_val = op.gdia_ptr<T>(); v.dia_ld = op.gdia_ld; v.ndiag = op.gndiag; v.dia_off = op.gdia_off.as<int32_t>();
  }
  return v;
}

// Term j of a stage: launch() enqueues the term kernel; an operator without a fused form is applied first (y = A x).
template <class L>
void taylor_term_launch(Ctx *c, Op &op, TaylorCall &tc, bool fused, const void *x, void *y, L &&launch) {
  if (fused) ++c->cnt_opapply;
  else op_apply_dev(op, x, y, nullptr, 0);
  {
    ProfScope ps(c, fused ? EXPV_MI_K_MATVEC : EXPV_MI_K_LINCOMB);
    launch();
  }
  ++tc.launches;
}

// info[0..7] / dinfo[0..3] of include/expv_mi.h from a call and the state it left
static inline void taylor_fill_info(const TaylorCall &tc, const dev::TaylorState &h, int64_t info[8], double dinfo[4]) {
  if (info) {
    info[0] = tc.m; info[1] = tc.s; info[2] = (int64_t)h.apps; info[3] = (int64_t)h.early; info[4] = tc.launches; info[5] = tc.reads;
    info[6] = tc.path; info[7] = (int64_t)h.nf_stage;
  }
  if (dinfo) { dinfo[0] = tc.alpha; dinfo[1] = tc.mu_re; dinfo[2] = tc.mu_im; dinfo[3] = f64_of(h.fnorm); }
}

// The launches of a single-column family behind a plan (tc): which form the operator takes, the arguments of a term that do not
// change from term to term, the grid, the closing launch and the term launch.
template <class T>
struct TaylorLaunch {
  Ctx *c;
  Op &op;
  TaylorCall &tc;
  T *F;
  dev::TaylorState *st;
  bool fused;
  int grid;      // of a term and of a closing launch: BLOCK / 64 slices of 64 packs per workgroup

  TaylorLaunch(Ctx *c_, Op &op_, TaylorCall &tc_, T *F_, dev::TaylorState *st_) : c(c_), op(op_), tc(tc_), F(F_), st(st_) {
    fused = taylor_fused(op);
    tc.path = fused ? 1 : 2;
    grid = dev::taylor_grid(op.n, dev::BLOCK * dev::Pack<T>::N);
  }
  dev::TaylorTermArgs<T> args() const {
    dev::TaylorTermArgs<T> a{};
    if (fused) a.op = taylor_op_view<T>(c, op);
    a.F = F; a.n = op.n; a.mu = taylor_scalar<T>(std::complex<double>(tc.mu_re, tc.mu_im)); a.tol = tc.tol; a.m = tc.m; a.st = st;
    return a;
  }
  // stage < 0: the first launch of a call (F = v = src, no scaling).  Otherwise F = eta F closes `stage`.  tail: see k_taylor_close.
  void close(const T *src, T *v, std::complex<double> eta, int64_t stage, double tail) const {
    const bool scale = stage >= 0 && !(eta.real() == 1.0 && eta.imag() == 0.0);
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_taylor_close<T>, dim3(grid), dim3(dev::BLOCK), 0, c->stream, src, F, v, op.n, taylor_scalar<T>(eta), scale ? 1 : 0,
                       (int)std::min<int64_t>(stage, 2147483646), (int)(stage + 1 < tc.s), tail, st);
  }
  // kernel(FUSED tag) names the instantiation: term(args, [](auto fused) { return k<T, decltype(fused)::value>; })
  template <class Args, class K>
  void term(const Args &args, const T *x, T *y, K &&kernel) const {
    taylor_term_launch(c, op, tc, fused, x, y, [&] {
      if (fused) hipLaunchKernelGGL(kernel(std::true_type()), dim3(grid), dim3(dev::BLOCK), 0, c->stream, args);
      else hipLaunchKernelGGL(kernel(std::false_type()), dim3(grid), dim3(dev::BLOCK), 0, c->stream, args);
    });
  }
};

}  // namespace expv_mi
