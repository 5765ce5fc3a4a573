// expv_taylor_realop.hip -- exp(tA)b by the truncated Taylor series for a REAL operator with a complex time and complex vectors
// (include/expv_mi.h: expv_mi_expv_taylor_realop): exp(-i t H) b with a real sparse H, a real Jacobian along a complex ray.  The
// operator is read in its own real type R -- no promoted copy, no imaginary halves that are all zero -- and the vectors have its
// complex counterpart C.
//
// A complex vector of n elements is an interleaved real block of n x 2, so (A x)_i is the block product of sparse_rows.h
// (RealOnComplex of realop_rows.h is BlockColumns<R, 2> with a row of one C), and everything behind it is the single call's: the element step
// taylor_step<C> with mu = (mu, 0), the closing kernel k_taylor_close<C>, the stage state, the arrival and the stopping test
// (taylor_state.h), the plan (expv_taylor.hip).  Two forms of a term:
//   path 1  the operator has a fused form (taylor_fused): k_taylor_term_realop walks the SELL slots or the general diagonal form of a
//           lane's Pack<R>::N rows against the interleaved x and does the element step in the same pass.  Per row and term: the
//           operator + the x gather, x_i and F read, y and F written.
//   path 2  everything else (overflow entries, column-blocked storage, dense, matrix-free): the operator's own real mul! on
//           the real plane and on the imaginary plane of v (two applications per term, each within the contract of a real n-vector),
//           then k_taylor_update_realop: the two product planes, x_i and F in, the element step, y, F and the two planes of the next v
//           out.  Three complex vectors and four real planes.
// gfx950 only.
#include <cmath>
#include <complex>

#include "engine.h"
#include "kernel_common.h"
#include "realop_rows.h"
#include "sparse_rows.h"
#include "taylor_state.h"
#include "taylor_term.h"

namespace expv_mi {
namespace dev {

template <class R>
struct RealOpTermArgs {
  using C = typename ComplexOf<R>::type;
  TaylorOpView<R> op;                             // (path 1)
  const R *ax_re, *ax_im;                         // (path 2) A Re(x) and A Im(x) as mul! left them
  R *v_re, *v_im;                                 // (path 2) the planes of the next v
  const C *x;                                     // v of the previous term
  C *y, *F;
  int64_t n;
  C c, mu;                                        // (t / s) / j and (tr(A) / n, 0)
  double tol;
  int j, m;
  TaylorState *st;
};

// the element step on the rows of a lane, the maxima over the rows below n
template <class R>
__device__ __forceinline__ void realop_rows(const RealOpTermArgs<R> &a, int64_t i, const R (*acc)[2], const CRows<typename ComplexOf<R>::type> &xi,
                                            CRows<typename ComplexOf<R>::type> &y, CRows<typename ComplexOf<R>::type> &f, double &mv, double &mf, unsigned &nan) {
  using C = typename ComplexOf<R>::type;
  constexpr int N = Pack<R>::N, NC = Pack<C>::N;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    C av, cv, fn;
    av.re = acc[k][0];
    av.im = acc[k][1];
    taylor_step(av, a.mu, xi.h[k / NC].v[k % NC], a.c, f.h[k / NC].v[k % NC], cv, fn);
    y.h[k / NC].v[k % NC] = cv;
    f.h[k / NC].v[k % NC] = fn;
    if (i + k < a.n) {      // (rows of the last pack beyond n hold what the padding slots gave: not part of the vector)
      note_abs(abs_T(cv), mv, nan, 1u);
      note_abs(abs_T(fn), mf, nan, 2u);
    }
  }
}

// path 1: thread (block, tid) takes the packs of whole slices, as the fused sweep of taylor_term.h does.  Q slots / diagonals in flight.
template <class R, int Q>
__global__ __launch_bounds__(BLOCK) void k_taylor_term_realop(RealOpTermArgs<R> a) {
  using C = typename ComplexOf<R>::type;
  constexpr int N = Pack<R>::N;
  constexpr int SH = 64 * N;
  static_assert(N == 2 * Pack<C>::N, "a lane's rows are two 16-byte packs of complex elements");
  if (taylor_skip(a.st)) return;
  double mv = 0.0, mf = 0.0;
  unsigned nan = 0u;
  const bool alx = is_al16(a.x), aly = is_al16(a.y), alf = is_al16(a.F);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nsl = (a.n + SH - 1) / SH;
  for (int64_t slice = (int64_t)blockIdx.x * (BLOCK / 64) + wave; slice < nsl; slice += (int64_t)gridDim.x * (BLOCK / 64)) {
    const int64_t i = slice * SH + (int64_t)lane * N;
    const CRows<C> xi = ld_crows(a.x, i, a.n, alx);      // independent of the operator: in flight with its slots
    CRows<C> f = ld_crows(a.F, i, a.n, alf), y;
    R acc[N][2];
    RealOnComplex<R> xs{a.x, acc};
    if (a.op.ndiag > 0) dia_walk<R, Q>(a.op.dia_val, a.op.dia_ld, a.op.ndiag, a.op.dia_off, i, a.n, xs);
    else sell_walk<R, Q>(a.op.A, slice, lane, xs);
    realop_rows<R>(a, i, acc, xi, y, f, mv, mf, nan);
    st_crows(a.y, i, a.n, aly, y);
    st_crows(a.F, i, a.n, alf, f);
  }
  if (taylor_arrive(a.st, mv, mf, nan) && threadIdx.x == 0) taylor_term_test(a.st, a.tol, a.j, a.m, 0.0);
}

// path 2: the update pass behind two real applications
template <class R>
__global__ __launch_bounds__(BLOCK) void k_taylor_update_realop(RealOpTermArgs<R> a) {
  using C = typename ComplexOf<R>::type;
  constexpr int N = Pack<R>::N;
  if (taylor_skip(a.st)) return;
  double mv = 0.0, mf = 0.0;
  unsigned nan = 0u;
  const bool alx = is_al16(a.x), aly = is_al16(a.y), alf = is_al16(a.F);
  const bool alp = is_al16(a.ax_re) && is_al16(a.ax_im), alv = is_al16(a.v_re) && is_al16(a.v_im);
  for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * N; i < a.n; i += (int64_t)gridDim.x * BLOCK * N) {
    const CRows<C> xi = ld_crows(a.x, i, a.n, alx);
    CRows<C> f = ld_crows(a.F, i, a.n, alf), y;
    const Pack<R> pr = ld_pack_user(a.ax_re, i, a.n, alp), pi = ld_pack_user(a.ax_im, i, a.n, alp);
    R acc[N][2];
#pragma unroll
    for (int k = 0; k < N; ++k) { acc[k][0] = pr.v[k]; acc[k][1] = pi.v[k]; }
    realop_rows<R>(a, i, acc, xi, y, f, mv, mf, nan);
    Pack<R> vr, vi;
#pragma unroll
    for (int k = 0; k < N; ++k) { vr.v[k] = y.h[k / Pack<C>::N].v[k % Pack<C>::N].re; vi.v[k] = y.h[k / Pack<C>::N].v[k % Pack<C>::N].im; }
    st_crows(a.y, i, a.n, aly, y);
    st_crows(a.F, i, a.n, alf, f);
    st_pack_user(a.v_re, i, a.n, alv, vr);
    st_pack_user(a.v_im, i, a.n, alv, vi);
  }
  if (taylor_arrive(a.st, mv, mf, nan) && threadIdx.x == 0) taylor_term_test(a.st, a.tol, a.j, a.m, 0.0);
}

}  // namespace dev

// the plan's kernels instantiated for the operator's real type, (m*, s) for the complex t, then every launch of the series
template <class R>
static void taylor_realop_run_T(Ctx *c, Op &op, std::complex<double> t, const void *b_dev, bool b_real, char *base, size_t head, size_t vbytes, size_t pbytes,
                                TaylorCall &tc) {
  using C = typename dev::ComplexOf<R>::type;
  constexpr int Q = 4;
  hipStream_t s = c->stream;
  const int64_t n = op.n, ns = tc.s;
  dev::TaylorState *st = reinterpret_cast<dev::TaylorState *>(base);
  C *V[2] = {reinterpret_cast<C *>(base + head), reinterpret_cast<C *>(base + head + vbytes)};
  C *F = reinterpret_cast<C *>(tc.F);
  const bool fused = taylor_fused(op);
  tc.path = fused ? 1 : 2;
  R *plane[4] = {nullptr, nullptr, nullptr, nullptr};      // Re v, Im v, A Re v, A Im v
  if (!fused)
    for (int k = 0; k < 4; ++k) plane[k] = reinterpret_cast<R *>(base + head + 3 * vbytes + (size_t)k * pbytes);
  const int grid_c = dev::taylor_grid(n, dev::BLOCK * dev::Pack<C>::N), grid_r = dev::taylor_grid(n, dev::BLOCK * dev::Pack<R>::N);
  const int grid_1 = dev::taylor_grid(n, dev::BLOCK);

  const C *src = reinterpret_cast<const C *>(b_dev);
  if (b_real) {      // F = (b, +0), and the series starts from F
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_realop_widen<R>, dim3(grid_1), dim3(dev::BLOCK), 0, s, reinterpret_cast<const R *>(b_dev), F, n);
    src = F;
  }
  const std::complex<double> eta = taylor_stage_factor(std::complex<double>(tc.mu_re, 0.0), t, ns);
  auto close = [&](const C *from, C *v, int64_t stage) {
    const bool scale = stage >= 0 && !(eta.real() == 1.0 && eta.imag() == 0.0);
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_taylor_close<C>, dim3(grid_c), dim3(dev::BLOCK), 0, s, from, F, v, n, taylor_scalar<C>(eta), scale ? 1 : 0,
                       (int)std::min<int64_t>(stage, 2147483646), (int)(stage + 1 < ns), 0.0, st);
    if (!fused && tc.m > 0 && stage + 1 < ns)
      hipLaunchKernelGGL(dev::k_realop_planes<R>, dim3(grid_1), dim3(dev::BLOCK), 0, s, v, plane[0], plane[1], n);
  };
  dev::RealOpTermArgs<R> a{};
  if (fused) a.op = taylor_op_view<R>(c, op);
  a.ax_re = plane[2]; a.ax_im = plane[3]; a.v_re = plane[0]; a.v_im = plane[1];
  a.F = F; a.n = n; a.mu = taylor_scalar<C>(std::complex<double>(tc.mu_re, 0.0)); a.tol = tc.tol; a.m = tc.m; a.st = st;
  int p = 0;
  close(src, V[0], -1);
  for (int64_t stage = 0; stage < ns; ++stage) {
    for (int j = 1; j <= tc.m; ++j) {
      a.x = V[p]; a.y = V[1 - p]; a.j = j;
      a.c = taylor_scalar<C>(t / (double)ns / (double)j);
      if (fused) {
        ++c->cnt_opapply;
        ProfScope ps(c, EXPV_MI_K_MATVEC);
        hipLaunchKernelGGL((dev::k_taylor_term_realop<R, Q>), dim3(grid_r), dim3(dev::BLOCK), 0, s, a);
      } else {
        op_apply_dev(op, plane[0], plane[2], nullptr, 0);
        op_apply_dev(op, plane[1], plane[3], nullptr, 0);
        ProfScope ps(c, EXPV_MI_K_LINCOMB);
        hipLaunchKernelGGL(dev::k_taylor_update_realop<R>, dim3(grid_r), dim3(dev::BLOCK), 0, s, a);
      }
      ++tc.launches;
      p ^= 1;
    }
    close(F, V[p], stage);
  }
  HIPCHECK(hipGetLastError());
}

void taylor_realop_enqueue(Ctx *c, Op &op, double t_re, double t_im, const void *b_dev, bool b_real, int precision, int64_t max_matvecs,
                           double opnorm, TaylorCall &tc) {
  c->use();
  try {
    const size_t csz = dtype_size(dtype_complex_of(op.dtype)), rsz = dtype_size(op.dtype);
    const size_t vbytes = up16((size_t)op.n * csz) + 16, pbytes = up16((size_t)op.n * rsz) + 16, head = taylor_head_bytes();
    tc.work.take_from(c, head + 3 * vbytes + (taylor_fused(op) ? 0 : 4 * pbytes));
    char *base = tc.work.as<char>();
    tc.state = base;
    tc.F = base + head + 2 * vbytes;
    taylor_shift_plan_realop(c, op, t_re, t_im, precision, max_matvecs, opnorm, base, tc);
    tc.mu_im = 0.0;
    if (op.dtype == EXPV_MI_F32) taylor_realop_run_T<float>(c, op, std::complex<double>(t_re, t_im), b_dev, b_real, base, head, vbytes, pbytes, tc);
    else taylor_realop_run_T<double>(c, op, std::complex<double>(t_re, t_im), b_dev, b_real, base, head, vbytes, pbytes, tc);
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);      // (the work vectors go back to the context: nothing may still be writing them)
    throw;
  }
}

}  // namespace expv_mi
