// krylov_realop.hip -- the Krylov step of a MIXED call: a real operator (F64 / F32) with a subspace and vectors of its complex
// counterpart (arnoldi! / lanczos! / expv / phiv_timestep! with a real sparse H and a complex psi: T = promote_type(eltype(A),
// eltype(b)) of the reference).  The operator is read in its own real type R -- no promoted copy, half the value bytes, one fma per
// component instead of a complex multiply whose second factor is half zeros -- and everything behind the product is the complex
// type's: projections, update, scale, combine.
//
//   k_spmv_realop       y = A x, real A on complex x / y: mul! of a mixed call on an operator with a fused form (taylor_fused)
//   k_fused_a2_realop   first kernel of the two-kernel step (fused.hip: k_fused_a2, plain loop) with y~ from the real operator walk
//   op_apply_mixed      mul! of a mixed call: the kernel above, or -- overflow rows, column-blocked storage, dense, matrix-free --
//                       the operator's own real mul! on the real and on the imaginary plane of x
// gfx950 only.
#include <algorithm>

#include "engine.h"
#include "kernel_common.h"
#include "realop_rows.h"
#include "sparse_rows.h"
#include "taylor_term.h"

namespace expv_mi {
namespace dev {

// the rows of a lane from the real operator: acc[k] = (A x)_{i + k} as (re, im)
template <class R, int Q>
__device__ __forceinline__ void realop_walk(const TaylorOpView<R> &op, int64_t slice, int lane, int64_t i, int64_t n,
                                            const typename ComplexOf<R>::type *__restrict__ x, R (*acc)[2]) {
  RealOnComplex<R> xs{x, acc};
  if (op.ndiag > 0) dia_walk<R, Q>(op.dia_val, op.dia_ld, op.ndiag, op.dia_off, i, n, xs);
  else sell_walk<R, Q>(op.A, slice, lane, xs);
}

// ---- mul!(y, A, x): one wave per SELL slice of the REAL type (64 Pack<R>::N rows), a lane owns Pack<R>::N rows = two 16-byte
// complex packs.  Per entry: one R of the operator, one C of x, one fma per component, in ascending stored order.  Rows < n only.
template <class R, int Q>
__global__ __launch_bounds__(BLOCK) void k_spmv_realop(TaylorOpView<R> op, int64_t n, const typename ComplexOf<R>::type *__restrict__ x,
                                                       typename ComplexOf<R>::type *__restrict__ y, const StepState *st, int step) {
  using C = typename ComplexOf<R>::type;
  constexpr int N = Pack<R>::N, NC = Pack<C>::N;
  constexpr int SH = 64 * N;
  static_assert(N == 2 * NC, "a lane's rows are two 16-byte packs of complex elements");
  if (step_skipped(st, step)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool aly = is_al16(y);
  const int64_t nsl = (n + SH - 1) / SH;
  for (int64_t slice = (int64_t)blockIdx.x * (BLOCK / 64) + wave; slice < nsl; slice += (int64_t)gridDim.x * (BLOCK / 64)) {
    const int64_t i = slice * SH + (int64_t)lane * N;
    R acc[N][2];
    realop_walk<R, Q>(op, slice, lane, i, n, x, acc);
    CRows<C> yv;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      yv.h[k / NC].v[k % NC].re = acc[k][0];
      yv.h[k / NC].v[k % NC].im = acc[k][1];
    }
    st_crows(y, i, n, aly, yv);
  }
}

// the planes of a complex vector and back (op_apply_mixed, path 2); both honour a finished factorisation like the operator kernels
template <class R>
__global__ __launch_bounds__(BLOCK) void k_realop_split(const typename ComplexOf<R>::type *__restrict__ z, R *__restrict__ re, R *__restrict__ im,
                                                        int64_t n, const StepState *st, int step) {
  using C = typename ComplexOf<R>::type;
  if (step_skipped(st, step)) return;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    const C v = z[i];
    re[i] = v.re;
    im[i] = v.im;
  }
}
template <class R>
__global__ __launch_bounds__(BLOCK) void k_realop_join(const R *__restrict__ re, const R *__restrict__ im, typename ComplexOf<R>::type *__restrict__ z,
                                                       int64_t n, const StepState *st, int step) {
  using C = typename ComplexOf<R>::type;
  if (step_skipped(st, step)) return;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    C v;
    v.re = re[i];
    v.im = im[i];
    z[i] = v;
  }
}

// ---- first kernel of the two-kernel step of a mixed call.  The plain loop of k_fused_a2<C, GRAM, DotChunk<C>::CH, DOTS_WAVES> with
// the slice geometry of the OPERATOR (a lane holds two complex packs) and y~ = A u_j from the real operator walk; the sums, their
// reduction and the epilogue are those of k_fused_a2.  A pack is touched only when it starts below n: the real type's slice may reach
// past the padded length of a complex column (Float32: 256 rows against 128).  Not here: augmentation, a caller's y~, overflow /
// column-blocked input, batching, the requests-up-front form.
// Waves per SIMD asked of the compiler: DOTS_WAVES like k_fused_a2, except for the Float32 operator with the Gram row -- ComplexF32
// packs against fp64 accumulators (two sets of 8 complex sums) do not fit 168 VGPRs beside a second pack's rows, and the kernel may
// not spill: two waves there.
template <class R, bool GRAM> struct RealopWaves { static constexpr int value = (sizeof(R) == 4 && GRAM) ? 2 : DOTS_WAVES; };
template <class R, bool GRAM>
__global__ __launch_bounds__(BLOCK, (RealopWaves<R, GRAM>::value)) void k_fused_a2_realop(FusedAArgs<typename ComplexOf<R>::type> fa, TaylorOpView<R> op, int spw, double tol) {
  using C = typename ComplexOf<R>::type;
  constexpr int N = Pack<R>::N, NC = Pack<C>::N;
  constexpr int SH = 64 * N;
  constexpr int CH = DotChunk<C>::CH;
  constexpr int NR = ST<C>::nreal;
  constexpr int NSETS = GRAM ? 2 : 1;
  constexpr int Q = 4;
  static_assert(N == 2 * NC, "a lane's rows are two 16-byte packs of complex elements");
  __shared__ double red_s[BLOCK / 64][CH * NR * NSETS];
  __shared__ double vals_s[MAX_RED_VALUES + 1];
  __shared__ double nrm_s[BLOCK / 64];
  __shared__ int flag_s;
  __shared__ C gs_s[GRAM ? (LOWSYNC_MAX * (LOWSYNC_MAX - 1) / 2) : 1];
  const DotsArgs<C> &a = fa.d;
  const C *u = fa.u;                       // V[:, jcol], unnormalised
  if (step_skipped(a.st, fa.step)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool al = ((a.ldv * sizeof(C)) % 16 == 0) && is_al16(a.V) && is_al16(fa.ybuf) && is_al16(u);
  const int64_t nsl = (a.n + SH - 1) / SH;
  double nrm = 0.0;
  for (int cb = 0; cb < a.nd; cb += CH) {
    using AT = typename ST<C>::acc_t;
    AT accd[CH], accg[GRAM ? CH : 1];
#pragma unroll
    for (int c = 0; c < CH; ++c) accd[c] = ST<AT>::zero();
    if (GRAM) {
#pragma unroll
      for (int c = 0; c < CH; ++c) accg[c] = ST<AT>::zero();
    }
    const int64_t s0 = ((int64_t)blockIdx.x * (BLOCK / 64) + wave) * spw;
    const int64_t s1 = (s0 + spw < nsl) ? s0 + spw : nsl;
    for (int64_t slice = s0; slice < s1; ++slice) {
      const int64_t i = slice * SH + (int64_t)lane * N;
      R acc[N][2];
      if (cb == 0) realop_walk<R, Q>(op, slice, lane, i, a.n, u, acc);      // y~ = A u_j for the lane's rows
      // one complex pack at a time (its u_j, its y~, its sums), so that a single pack's operands are live beside the accumulators
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t ih = i + h * NC;
        if (ih < a.n) {
          const Pack<C> xv = ld_pack(u, ih, a.n, al);
          Pack<C> yv;
          if (cb == 0) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
              C v;
              v.re = acc[h * NC + k][0];
              v.im = acc[h * NC + k][1];
              yv.v[k] = (ih + k < a.n) ? v : ST<C>::zero();      // rows past n: zero in the sums and in the padding of y~
              nrm += ST<C>::abs2(xv.v[k]);
            }
            st_pack(fa.ybuf, ih, a.n, al, yv);
          } else {
            yv = ld_pack(fa.ybuf, ih, a.n, al);
          }
          dots_accumulate<C, GRAM, CH>(a.V, a.ldv, a.n, a.c0, a.dir, a.nd, cb, ih, al, yv, xv, accd, accg);
        }
      }
    }
    dots_publish_chunk<C, GRAM, CH>(accd, accg, cb, a.nd, a.part, red_s);
  }
  const int NV = a.nd * NR * NSETS;        // index of the extra value ||u_j||^2
  const double bs = block_sum(nrm, nrm_s);
  if (threadIdx.x == 0) publish_f64(a.part + (size_t)NV * MAX_GRID + blockIdx.x, bs);
  if (!hier_reduce(a.st, a.part, a.gpart, NV + 1, vals_s, &flag_s)) return;

  // ---- last workgroup: finish step j-1 (norm, breakdown) and produce the column of step j (k_fused_a2's epilogue) -------
  const double beta = fa.cont ? 1.0 : sqrt(vals_s[NV]);
  const double inv = fa.cont ? 1.0 : 1.0 / beta;
  const int jcol = a.jcol;
  bool stop = false;
  if (fa.cont) stop = false;
  else if (fa.step == 1) stop = (beta == 0.0);             // iszero(Ks.beta) && return  (arnoldi.jl:366)
  else stop = (beta < tol);                                // happy breakdown of step j-1  (arnoldi.jl:370)
  if (threadIdx.x == 0) {
    if (!fa.cont) a.st->hnorm = beta;
    a.st->inv = inv;
    a.st->m_done = fa.step - 1;
    if (fa.cont) {
    } else if (fa.step == 1) a.st->beta0sq = vals_s[NV];
    else a.Hdev[jcol + (int64_t)(jcol - 1) * a.ldh] = ST<C>::from_real(beta);   // H[j, j-1] = ||u_j||
    if (stop) a.st->breakdown = (fa.step == 1) ? 2 : 1;
  }
  if (stop) return;
  for (int e = threadIdx.x; e < NV; e += BLOCK) {
    const int set = e / (a.nd * NR), col = (e % (a.nd * NR)) / NR;
    const double f = (set == 0 && col == a.nd - 1) ? inv * inv : inv;
    vals_s[e] *= f;
  }
  __syncthreads();
  projection_epilogue<C>(a, vals_s, gs_s, inv);
}

}  // namespace dev

template <class R> struct RealOfDev;
template <> struct RealOfDev<cplx> { using type = double; };
template <> struct RealOfDev<cplx32> { using type = float; };

template <class C>
void fused_a2_realop(Ctx *c, const Op &op, const dev::FusedAArgs<C> &fa, double tol) {
  using R = typename RealOfDev<C>::type;
  const dev::TaylorOpView<R> view = taylor_op_view<R>(c, op);
  const int64_t nslices = op.nslices;      // the operator's own slices (64 Pack<R>::N rows each): a mixed call is never augmented
  int nb, spw;
  if (fa.d.mode == dev::DOTS_LOWSYNC) {
    auto k = dev::k_fused_a2_realop<R, true>;
    dev::plan_slices(nslices, std::max(1, dev::resident_blocks((const void *)k)), &nb, &spw);
    hipLaunchKernelGGL(k, dim3(nb), dim3(dev::BLOCK), 0, c->stream, fa, view, spw, tol);
  } else {
    auto k = dev::k_fused_a2_realop<R, false>;
    dev::plan_slices(nslices, std::max(1, dev::resident_blocks((const void *)k)), &nb, &spw);
    hipLaunchKernelGGL(k, dim3(nb), dim3(dev::BLOCK), 0, c->stream, fa, view, spw, tol);
  }
}
template void fused_a2_realop<cplx>(Ctx *, const Op &, const dev::FusedAArgs<cplx> &, double);
template void fused_a2_realop<cplx32>(Ctx *, const Op &, const dev::FusedAArgs<cplx32> &, double);

template <class R>
static void op_apply_mixed_T(Op &op, const typename dev::ComplexOf<R>::type *x, typename dev::ComplexOf<R>::type *y, const StepState *st, int step,
                             DevBuf &work) {
  Ctx *c = op.ctx;
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  if (n <= 0) return;
  if (taylor_fused(op)) {      // path 1: the operator walked against the interleaved x
    constexpr int SH = 64 * dev::Pack<R>::N;
    ++c->cnt_opapply;
    ProfScope ps(c, EXPV_MI_K_MATVEC);
    int64_t g = ((n + SH - 1) / SH + (dev::BLOCK / 64) - 1) / (dev::BLOCK / 64);
    g = std::min<int64_t>(std::max<int64_t>(g, 1), dev::MAX_GRID);
    hipLaunchKernelGGL((dev::k_spmv_realop<R, 4>), dim3((int)g), dim3(dev::BLOCK), 0, s, taylor_op_view<R>(c, op), n, x, y, st, step);
    return;
  }
  // path 2: the operator's own real mul! on each plane (a matrix-free callback sees real n-vectors), then the planes joined
  const size_t pbytes = ((size_t)n * sizeof(R) + 15) / 16 * 16 + 16;
  if (work.bytes < 4 * pbytes) work.take_from(c, 4 * pbytes);
  R *plane[4];
  for (int k = 0; k < 4; ++k) plane[k] = reinterpret_cast<R *>(work.as<char>() + (size_t)k * pbytes);
  const int grid = dev::grid_for(n, dev::BLOCK);
  {
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_realop_split<R>, dim3(grid), dim3(dev::BLOCK), 0, s, x, plane[0], plane[1], n, st, step);
  }
  op_apply_dev(op, plane[0], plane[2], st, step);
  op_apply_dev(op, plane[1], plane[3], st, step);
  ProfScope ps(c, EXPV_MI_K_LINCOMB);
  hipLaunchKernelGGL(dev::k_realop_join<R>, dim3(grid), dim3(dev::BLOCK), 0, s, plane[2], plane[3], y, n, st, step);
}

void op_apply_mixed(Op &op, const void *x_dev, void *y_dev, const StepState *st, int step, DevBuf &work) {
  if (op.dtype == EXPV_MI_F32) op_apply_mixed_T<float>(op, (const cplx32 *)x_dev, (cplx32 *)y_dev, st, step, work);
  else if (op.dtype == EXPV_MI_F64) op_apply_mixed_T<double>(op, (const cplx *)x_dev, (cplx *)y_dev, st, step, work);
  else fail(EXPV_MI_ARGUMENT_ERROR, "op_apply_complex: the operator is complex; expv_mi_op_apply is the call for a complex operator");
  HIPCHECK(hipGetLastError());
}

}  // namespace expv_mi
