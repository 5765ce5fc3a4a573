// expv_taylor_grid.hip -- exp(r_k t A) b for nt multipliers r_k >= 0 in ONE sweep of the truncated Taylor series of expv_taylor.hip.
//
// R = max r_k, T = R t;  (mu, alpha, m*, s) are those of the single call for T, h = T / s.  Output k is classified in double:
//     x_k = s (r_k / R),  i_k = max(ceil(x_k) - 1, 0),  rho_k = x_k - i_k
//   r_k = 0    the output is b;
//   rho_k = 1  a STAGE-END output: a copy of F after stage i_k has closed;
//   otherwise  an INTERIOR output of stage i_k: the terms v_j = (hA)^j F / j! of the stage are all there, and
//              exp(rho h A) F = sum_j rho^j v_j, so G_k = F + sum_j d_kj v_j with d_kj = d_k,j-1 rho_k (double, rounded to the
//              operator's real type, passed by value), closed with G_k <- exp(mu rho_k h) G_k.
// F and v run through the row sweep and the element step of the single call (taylor_sweep, taylor_term.h; taylor_step,
// taylor_state.h) with the panel as the sweep's policy: every output with r_k = R is bit for bit what the single call returns for T.  No output costs a pass over the operator: the interior outputs of a stage live
// in panels of P in {2, 4, 8} interleaved columns [row][P]; the first panel is updated in the epilogue of the term kernel, every
// further one by an accumulate-only launch that reads v_j once for its panel.
//
// Stopping.  Output k: c2 = d_kj |v_j|_inf, c1 starts as the stage's c1, stop when c1 + c2 <= tol |G_k|_inf, else c1 = c2.  A stopped
// output is masked (written back unchanged, no maxima); so is F once its own test has passed.  v_j keeps being computed while F or
// any output of the stage is live; a term launch returns at once when all of them have stopped or the call has ended.  An interior
// output that took no term (a zero F, a call that a non-finite F ended earlier) is F as it stands.
//
// Synchronisation is that of expv_taylor.hip: agent-scope atomic maxima / OR, one ticket per launch, lane 0 of the last workgroup
// to arrive runs the tests and re-arms the state through L1-bypassing accesses.  A stage that has outputs keeps a TaylorGridStage
// (the stage's c1, |v_j|_inf of the last term, the count of live outputs over all its panels, the terms F took) and one
// TaylorGridPanel per panel; the host writes their initial values once and reads them back with the final state.
#include <cmath>
#include <complex>
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <vector>

#include "engine.h"
#include "kernel_common.h"
#include "taylor_state.h"
#include "taylor_term.h"

namespace expv_mi {
namespace dev {

constexpr int GPANEL = 8;      // columns of a full panel; a remainder runs in the smallest P in {2, 4, 8} that holds it

struct TaylorGridPanel {      // 32 words of 8 bytes; the access rules are those of TaylorState
  unsigned long long maxg[GPANEL];      // running maxima of |G_ik| per column
  unsigned long long c1[GPANEL];
  unsigned long long terms[GPANEL];     // terms that entered G_k
  unsigned long long nang;              // bit k: a NaN among G_k
  unsigned long long ticket;            // of the accumulate-only launches (the first panel arrives on the stage state's ticket)
  unsigned long long stopped;           // bit k (padding columns: set from the start)
  unsigned long long spare[5];
};
static_assert(sizeof(TaylorGridPanel) == 256, "TaylorGridPanel layout");
struct TaylorGridStage {      // 8 words
  unsigned long long c1;                // |F|_inf when the stage began
  unsigned long long vmax;              // |v_j|_inf of the last term launch (NaN when v held one)
  unsigned long long live;              // interior outputs of the stage that have not stopped, over all panels
  unsigned long long fterms;            // terms that entered F in this stage
  unsigned long long spare[4];
};
static_assert(sizeof(TaylorGridStage) == 64, "TaylorGridStage layout");

template <class T, int P>
struct __attribute__((aligned(16))) GridRow {
  static_assert(P * sizeof(T) % 16 == 0, "a row of a panel is a whole number of 16-byte packs");
  T v[P];
};

__device__ __forceinline__ unsigned grid_uniform(unsigned long long v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v); }

// A running maximum of absolute values that KEEPS a NaN: a non-negative double orders like its bit pattern, and the pattern of a
// NaN lies above that of infinity -- one compare per value where note_abs needs two and a mask per column.  The sign bit is
// cleared first: nothing promises that the NaN a modulus returns is a positive one.  grid_arrive turns a NaN maximum into the
// column's NaN bit.
__device__ __forceinline__ void note_abs_nan(double a, double &m) {
  const long long ua = __double_as_longlong(a) & 0x7fffffffffffffffll;
  m = ua > __double_as_longlong(m) ? __longlong_as_double(ua) : m;
}

// g + d v with a real d: one fused multiply-add per real component
__device__ __forceinline__ double grid_axpy(double d, double v, double g) { return fma(d, v, g); }
__device__ __forceinline__ float grid_axpy(float d, float v, float g) { return fmaf(d, v, g); }
__device__ __forceinline__ cplx grid_axpy(double d, cplx v, cplx g) { return make_cplx(fma(d, v.re, g.re), fma(d, v.im, g.im)); }
__device__ __forceinline__ cplx32 grid_axpy(float d, cplx32 v, cplx32 g) { return make_cplx32(fmaf(d, v.re, g.re), fmaf(d, v.im, g.im)); }

template <class T>
struct GridCoef {
  typename ST<T>::real_t d[GPANEL];      // d_kj of the panel's columns
};

template <class T>
struct GridTermArgs {
  TaylorTermArgs<T> t;
  T *G;                                  // the first panel of the stage, [row][P]
  GridCoef<T> co;
  TaylorGridPanel *ps;
  TaylorGridStage *gs;
};

// The coefficients of a term kernel's panel wait in LDS for the epilogue: by value they would sit in 2 P scalar registers through
// the operator loop, which is short of them (the compiler's resource report: spills at P = 8).
template <class T, int P>
__device__ __forceinline__ void grid_coef_to_lds(typename ST<T>::real_t (&d_s)[P], const GridCoef<T> &co) {
#pragma unroll
  for (int p = 0; p < P; ++p)
    if (threadIdx.x == (unsigned)p) d_s[p] = co.d[p];
  __syncthreads();
}

// One row of a panel: G_k += d_k v for the live columns (term 1: G_k = x0 + d_k v, x0 = F as the stage began = v_0), maxima.
template <class T, int P>
__device__ __forceinline__ void grid_panel_row(T *G, int64_t row, bool first, T x0, T v, const typename ST<T>::real_t *d, unsigned off,
                                               double (&mg)[P]) {
  using Row = GridRow<T, P>;
  Row g;
  if (first) {
#pragma unroll
    for (int p = 0; p < P; ++p) g.v[p] = x0;
  } else {
    g = *reinterpret_cast<const Row *>(G + row * P);
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if ((off >> p) & 1u) continue;      // (a masked column: written back as it is)
    g.v[p] = grid_axpy(d[p], v, g.v[p]);
    note_abs_nan(abs_T(g.v[p]), mg[p]);
    // (P = 8: column by column.  Left to interleave eight moduli the compiler takes 111 instead of 94 vector registers for
    // k_taylor_term_grid<ComplexF64, 8> -- its resource report -- which costs a wave per SIMD.)
    if constexpr (P == 8) __builtin_amdgcn_sched_barrier(0);
  }
  *reinterpret_cast<Row *>(G + row * P) = g;
}

// taylor_arrive + the P column maxima of a panel: this workgroup's maxima into the states, then one ticket.  st == nullptr: an
// accumulate-only launch (no v, no F).
template <int P>
__device__ __forceinline__ bool grid_arrive(TaylorState *st, TaylorGridPanel *ps, unsigned long long *ticket, double mv, double mf, unsigned nan,
                                            double (&mg)[P]) {
  unsigned nang = 0u;
#pragma unroll
  for (int p = 0; p < P; ++p)
    if (mg[p] != mg[p]) { nang |= 1u << p; mg[p] = 0.0; }
  __shared__ double m_s[BLOCK / 64][P + 2];
  __shared__ unsigned nan_s[BLOCK / 64][2];
  __shared__ int last_s;
  mv = wave_max(mv);
  mf = wave_max(mf);
  nan = (__any((int)(nan & 1u)) ? 1u : 0u) | (__any((int)(nan & 2u)) ? 2u : 0u);
  unsigned wg = 0u;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    mg[p] = wave_max(mg[p]);
    wg |= __any((int)((nang >> p) & 1u)) ? (1u << p) : 0u;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int p = 0; p < P; ++p) m_s[wave][p] = mg[p];
    m_s[wave][P] = mv;
    m_s[wave][P + 1] = mf;
    nan_s[wave][0] = nan;
    nan_s[wave][1] = wg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) {
#pragma unroll
      for (int p = 0; p < P; ++p) mg[p] = fmax(mg[p], m_s[w][p]);
      mv = fmax(mv, m_s[w][P]);
      mf = fmax(mf, m_s[w][P + 1]);
      nan |= nan_s[w][0];
      wg |= nan_s[w][1];
    }
    if (st) {
      if (mv > 0.0) atomicMax(&st->maxv, (unsigned long long)__double_as_longlong(mv));
      if (mf > 0.0) atomicMax(&st->maxf, (unsigned long long)__double_as_longlong(mf));
      if (nan) atomicOr(&st->nanflags, (unsigned long long)nan);
    }
#pragma unroll
    for (int p = 0; p < P; ++p)
      if (mg[p] > 0.0) atomicMax(&ps->maxg[p], (unsigned long long)__double_as_longlong(mg[p]));
    if (wg) atomicOr(&ps->nang, (unsigned long long)wg);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = (t == (unsigned long long)gridDim.x - 1ull);
  }
  __syncthreads();
  return last_s != 0;
}

// lane 0 of the last workgroup: the tests of a panel's live columns against |v_j|_inf in gs->vmax, then the panel re-armed
template <class T, int P>
__device__ __forceinline__ void grid_panel_test(TaylorGridPanel *ps, TaylorGridStage *gs, const typename ST<T>::real_t *d, double tol, int j) {
  const double vmax = ts_loadf(&gs->vmax);
  const unsigned long long ng = ts_load(&ps->nang);
  unsigned long long stopped = ts_load(&ps->stopped), live = ts_load(&gs->live);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (!((stopped >> p) & 1ull)) {
      const double c2 = (double)d[p] * vmax;
      const double gn = ((ng >> p) & 1ull) ? taylor_qnan() : ts_loadf(&ps->maxg[p]);
      const double c1 = ts_loadf(j == 1 ? &gs->c1 : &ps->c1[p]);
      ts_store(&ps->terms[p], ts_load(&ps->terms[p]) + 1ull);
      if (c1 + c2 <= tol * gn) {
        stopped |= 1ull << p;
        --live;
      } else {
        ts_storef(&ps->c1[p], c2);
      }
    }
    ts_store(&ps->maxg[p], 0ull);
  }
  ts_store(&ps->stopped, stopped);
  ts_store(&gs->live, live);
  ts_store(&ps->nang, 0ull);
  ts_store(&ps->ticket, 0ull);
}

// lane 0 of the last workgroup of a term launch: |v_j|_inf for the panels, F's test (unless F has stopped), then the first panel's
template <class T, int P>
__device__ __forceinline__ void grid_term_test(const GridTermArgs<T> &ga, const typename ST<T>::real_t *d, bool fstop, bool pan) {
  const TaylorTermArgs<T> &a = ga.t;
  TaylorState *st = a.st;
  TaylorGridStage *gs = ga.gs;
  const unsigned long long nan = ts_load(&st->nanflags);
  const double c2 = taylor_vmax(st, nan);
  if (a.j == 1) ts_store(&gs->c1, ts_load(&st->c1));      // (before F's test replaces it)
  ts_storef(&gs->vmax, c2);
  ts_store(&st->apps, ts_load(&st->apps) + 1ull);
  if (!fstop) {
    const double fn = taylor_fnorm(st, nan);
    const double c1 = ts_loadf(&st->c1);
    ts_store(&gs->fterms, ts_load(&gs->fterms) + 1ull);
    taylor_f_test(st, c1, c2, fn, a.tol, a.j, a.m);
  }
  if (pan) grid_panel_test<T, P>(ga.ps, gs, d, a.tol, a.j);
  taylor_rearm(st);
}

// Nothing left to do in this launch: the call has ended, F has stopped and so has every output of the stage, or F is zero (the
// closing launch marks a zero F as stopped: only then is `stopped` set before term 1 -- nothing is applied, and the outputs of the
// stage count as stopped from here on).
__device__ __forceinline__ bool grid_skip(const TaylorState *st, TaylorGridStage *gs, int j) {
  if (ts_load(&st->ended) != 0ull) return true;
  if (ts_load(&st->stopped) == 0ull) return false;
  if (j == 1) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ts_store(&gs->live, 0ull);
    return true;
  }
  return ts_load(&gs->live) == 0ull;
}

// The first panel of the stage's interior outputs as a policy of taylor_sweep: F masked once it has stopped, and the panel's rows
// updated behind the stores of y and F.
template <class T, int P>
struct GridPanel {
  const GridTermArgs<T> &ga;
  const typename ST<T>::real_t *d;      // the panel's coefficients, in LDS
  const bool fstop;
  const unsigned off;                   // the panel's stopped columns
  const bool pan;                       // a column of the panel is live
  double mg[P];
  __device__ __forceinline__ void rows(int64_t i, const Pack<T> &xi, const Pack<T> &y) {
    if (!pan) return;
#pragma unroll
    for (int k = 0; k < Pack<T>::N; ++k)
      if (i + k < ga.t.n) grid_panel_row<T, P>(ga.G, i + k, ga.t.j == 1, xi.v[k], y.v[k], d, off, mg);
  }
};

// k_taylor_term + the first panel of the stage's interior outputs
template <class T, int P, bool FUSED>
__global__ __launch_bounds__(BLOCK) void k_taylor_term_grid(GridTermArgs<T> ga) {
  const TaylorTermArgs<T> &a = ga.t;
  if (grid_skip(a.st, ga.gs, a.j)) return;
  constexpr unsigned ALL = (1u << P) - 1u;
  const bool fstop = grid_uniform(ts_load(&a.st->stopped)) != 0u;
  const unsigned off = grid_uniform(ts_load(&ga.ps->stopped)) & ALL;
  __shared__ typename ST<T>::real_t d_s[P];
  grid_coef_to_lds<T, P>(d_s, ga.co);
  GridPanel<T, P> x{ga, d_s, fstop, off, off != ALL, {}};
  double mv = 0.0, mf = 0.0;
  unsigned nan = 0u;
  taylor_sweep<T, FUSED>(a, x, mv, mf, nan);
  if (grid_arrive<P>(a.st, ga.ps, &a.st->ticket, mv, mf, nan, x.mg) && threadIdx.x == 0) grid_term_test<T, P>(ga, d_s, fstop, x.pan);
}

template <class T>
struct GridAccumArgs {
  const T *x, *y;      // v_{j-1} (term 1: F as the stage began) and v_j, as the term launch left them
  T *G;
  int64_t n;
  GridCoef<T> co;
  double tol;
  int j;
  const TaylorState *st;
  TaylorGridPanel *ps;
  TaylorGridStage *gs;
};

// A further panel of a stage with more than 8 interior outputs: v_j is read once for the panel's columns.  It runs behind the
// term launch of the same j, which has left |v_j|_inf in the stage state.
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_taylor_grid_accum(GridAccumArgs<T> a) {
  constexpr unsigned ALL = (1u << P) - 1u;
  if (ts_load(&a.st->ended) != 0ull || ts_load(&a.gs->live) == 0ull) return;
  const unsigned off = grid_uniform(ts_load(&a.ps->stopped)) & ALL;
  if (off == ALL) return;
  double mg[P];
#pragma unroll
  for (int p = 0; p < P; ++p) mg[p] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * BLOCK)
    grid_panel_row<T, P>(a.G, r, a.j == 1, a.j == 1 ? a.x[r] : ST<T>::zero(), a.y[r], a.co.d, off, mg);
  if (grid_arrive<P>(nullptr, a.ps, &a.ps->ticket, 0.0, 0.0, 0u, mg) && threadIdx.x == 0) grid_panel_test<T, P>(a.ps, a.gs, a.co.d, a.tol, a.j);
}

template <class T>
struct GridOutArgs {
  const T *src;                  // a panel [row][P] (ps != nullptr) or a vector (b, F) that goes to every column listed
  const T *F;                    // what an interior output that took no term is
  const TaylorGridPanel *ps;
  int pc;                        // columns in use
  int col[GPANEL];               // the column of W each of them goes to
  T scale[GPANEL];
  unsigned scaled;               // bit p: multiply by scale[p]
  const int32_t *pinv;           // a reordered operator: row r of the caller is row pinv[r] here
  T *W;
  int64_t rs, cs, n;             // element (i, k) of W at W[i rs + k cs]
};

// Closes outputs: the per-column scale, rows back into the caller's ordering, a strided store into W.
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_taylor_grid_out(GridOutArgs<T> a) {
  using Row = GridRow<T, P>;
  __shared__ T scale_s[P];      // (by value they would not fit the scalar registers beside the rest: the resource report)
  __shared__ int64_t col_s[P];
#pragma unroll
  for (int p = 0; p < P; ++p)
    if (threadIdx.x == (unsigned)p) { scale_s[p] = a.scale[p]; col_s[p] = (int64_t)a.col[p] * a.cs; }
  __syncthreads();
  unsigned fb = 0u;      // columns that took no term: F as it stands
  if (a.ps) {
#pragma unroll
    for (int p = 0; p < P; ++p) fb |= ts_load(&a.ps->terms[p]) == 0ull ? (1u << p) : 0u;
    fb = grid_uniform(fb);
  }
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * BLOCK) {
    const int64_t q = a.pinv ? (int64_t)a.pinv[r] : r;
    Row g;
    if (a.ps) {
      g = *reinterpret_cast<const Row *>(a.src + q * P);
    } else {
      const T s = a.src[q];
#pragma unroll
      for (int p = 0; p < P; ++p) g.v[p] = s;
    }
    T fv = ST<T>::zero();
    if (fb) fv = a.F[q];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (p >= a.pc) continue;
      T v = g.v[p];
      if ((fb >> p) & 1u) v = fv;
      else if ((a.scaled >> p) & 1u) v = mul_as_single(scale_s[p], v);
      a.W[r * a.rs + col_s[p]] = v;
    }
  }
}

}  // namespace dev

// ------------------------------------------------------------------------------------------
// the classification (host only)
// ------------------------------------------------------------------------------------------
void taylor_grid_plan(int64_t s, const double *r, int nt, int64_t *stage, double *rho, int *kind) {
  if (nt < 0) fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor_grid: nt = " + std::to_string(nt) + " is negative");
  if (s < 1) fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor_grid: s = " + std::to_string(s) + " stages");
  if (nt > 0 && !r) fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor_grid: null pointer");
  double R = 0.0;
  for (int k = 0; k < nt; ++k) {
    if (!(r[k] >= 0.0) || !std::isfinite(r[k]))
      fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor_grid: multiplier " + std::to_string(k) + " = " + std::to_string(r[k]) + " is not a finite non-negative number");
    R = std::max(R, r[k]);
  }
  for (int k = 0; k < nt; ++k) {
    int64_t i = -1;
    double ro = 0.0;
    int kd = 0;
    if (r[k] != 0.0) {
      const double x = (double)s * (r[k] / R);
      const double id = std::max(std::ceil(x) - 1.0, 0.0);
      i = (int64_t)id;
      ro = x - id;
      kd = ro == 1.0 ? 2 : 1;
    }
    if (stage) stage[k] = i;
    if (rho) rho[k] = ro;
    if (kind) kind[k] = kd;
  }
}

namespace {

struct GridStagePlan {      // a stage that has outputs
  int64_t stage;
  std::vector<int> interior, ends;
  size_t state_off = 0;      // of its TaylorGridStage in the state block; its panels follow
};

// the smallest P in {2, 4, 8} that holds pc columns in whole 16-byte packs of T
template <class T> int panel_width(int pc) {
  constexpr int PMIN = (16 / (int)sizeof(T)) > 2 ? 16 / (int)sizeof(T) : 2;
  return std::max(PMIN, pc <= 2 ? 2 : pc <= 4 ? 4 : 8);
}
// f(integral_constant<int, P>) for the P that panel_width gave
template <class T, class F> void with_panel(int P, F &&f) {
  if constexpr (sizeof(T) >= 8) {
    if (P == 2) { f(std::integral_constant<int, 2>()); return; }
  }
  if (P == 4) f(std::integral_constant<int, 4>());
  else f(std::integral_constant<int, 8>());
}

template <class T>
void grid_run_T(Ctx *c, Op &op, std::complex<double> t, const double *r, int nt, const T *b_dev, T *Wd, int64_t rs, int64_t cs, int precision,
                int64_t max_matvecs, double opnorm, const std::function<void()> &before_wait, int64_t info[10], double dinfo[4], int64_t *col_info) {
  using real_t = typename ST<T>::real_t;
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  double R = 0.0;
  for (int k = 0; k < nt; ++k) R = std::max(R, r[k]);
  const std::complex<double> Tt = R * t;

  // Everything a queued launch or copy may still touch, declared ahead of the guard that waits for the stream when an error
  // unwinds this frame: the guard is destroyed first, the buffers go back to the context (and the host vectors away) after it.
  TaylorCall tc;
  DevBuf head, work;
  std::vector<unsigned long long> init, hs;
  dev::TaylorState hst;
  struct SyncOnUnwind {
    hipStream_t s;
    int pending = std::uncaught_exceptions();
    ~SyncOnUnwind() { if (std::uncaught_exceptions() > pending) (void)hipStreamSynchronize(s); }
  } sync_on_unwind{s};
  head.take_from(c, taylor_head_bytes());
  taylor_shift_plan(c, op, Tt.real(), Tt.imag(), precision, max_matvecs, opnorm, head.p, tc);      // (a refusal: nothing has touched W)
  const std::complex<double> mu(tc.mu_re, tc.mu_im);
  const int m = tc.m;
  const int64_t ns = tc.s;

  // the outputs by stage
  std::vector<int64_t> stage((size_t)nt);
  std::vector<double> rho((size_t)nt);
  std::vector<int> kind((size_t)nt);
  taylor_grid_plan(ns, r, nt, stage.data(), rho.data(), kind.data());
  std::vector<int> order;
  std::vector<int> from_b;
  for (int k = 0; k < nt; ++k) (kind[k] == 0 ? from_b : order).push_back(k);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return stage[a] < stage[b]; });
  std::vector<GridStagePlan> plans;
  for (int k : order) {
    if (plans.empty() || plans.back().stage != stage[k]) { plans.emplace_back(); plans.back().stage = stage[k]; }
    // without a term there is no panel: alpha = 0 closes its interior outputs from b
    (kind[k] == 1 ? plans.back().interior : plans.back().ends).push_back(k);
  }
  int qmax = 0, qpan = 0;
  // (a stage without outputs runs the same kernels on a state block of its own, shared by all such stages: no live output ever)
  size_t sbytes = sizeof(dev::TaylorGridStage) + sizeof(dev::TaylorGridPanel);
  for (auto &pl : plans) {
    const int q = m > 0 ? (int)pl.interior.size() : 0;      // (alpha = 0: no term, no panel)
    qmax = std::max(qmax, (int)pl.interior.size());
    qpan = std::max(qpan, q);
    pl.state_off = sbytes;
    sbytes += sizeof(dev::TaylorGridStage) + sizeof(dev::TaylorGridPanel) * (size_t)std::max(1, (q + dev::GPANEL - 1) / dev::GPANEL);
  }
  const int npan_max = (qpan + dev::GPANEL - 1) / dev::GPANEL;

  // workspace: the states, the three vectors of the single call, the panels
  const size_t vbytes = up16((size_t)n * sizeof(T)) + 16, pbytes = up16((size_t)n * dev::GPANEL * sizeof(T));
  work.take_from(c, up16(sbytes) + 16 + 3 * vbytes + (size_t)npan_max * pbytes);
  char *base = work.as<char>();
  char *states = base;
  T *V[2] = {reinterpret_cast<T *>(base + up16(sbytes) + 16), reinterpret_cast<T *>(base + up16(sbytes) + 16 + vbytes)};
  T *F = reinterpret_cast<T *>(base + up16(sbytes) + 16 + 2 * vbytes);
  char *panels = base + up16(sbytes) + 16 + 3 * vbytes;
  dev::TaylorState *st = reinterpret_cast<dev::TaylorState *>(head.p);

  init.assign(sbytes / 8, 0ull);
  {
    dev::TaylorGridPanel ps{};
    ps.stopped = ~0ull;
    std::memcpy(reinterpret_cast<char *>(init.data()) + sizeof(dev::TaylorGridStage), &ps, sizeof(ps));
  }
  for (auto &pl : plans) {
    const int q = m > 0 ? (int)pl.interior.size() : 0;
    dev::TaylorGridStage gs{};
    gs.live = (unsigned long long)q;
    std::memcpy(reinterpret_cast<char *>(init.data()) + pl.state_off, &gs, sizeof(gs));
    const int np = std::max(1, (q + dev::GPANEL - 1) / dev::GPANEL);
    for (int pi = 0; pi < np; ++pi) {
      dev::TaylorGridPanel ps{};
      const int pc = std::max(0, std::min(dev::GPANEL, q - pi * dev::GPANEL));
      ps.stopped = ~((1ull << pc) - 1ull);
      std::memcpy(reinterpret_cast<char *>(init.data()) + pl.state_off + sizeof(gs) + sizeof(ps) * (size_t)pi, &ps, sizeof(ps));
    }
  }
  HIPCHECK(hipMemcpyAsync(states, init.data(), sbytes, hipMemcpyHostToDevice, s));

  const TaylorLaunch<T> L(c, op, tc, F, st);
  dev::GridTermArgs<T> ga{};
  dev::TaylorTermArgs<T> &a = ga.t;
  a = L.args();
  const int g_rows = dev::taylor_grid(n, dev::BLOCK);
  const std::complex<double> h = Tt / (double)ns;
  const std::complex<double> eta = taylor_stage_factor(mu, Tt, ns);
  const int32_t *pinv = op.perm ? op.perm->pinv.as<int32_t>() : nullptr;
  int64_t accum_launches = 0;

  // the outputs `cols` from a vector (b or F), 8 per launch; factor[k]: what output k is multiplied by
  auto out_vector = [&](const T *src, const std::vector<int> &cols, const std::vector<std::complex<double>> *factor) {
    for (size_t k0 = 0; k0 < cols.size(); k0 += dev::GPANEL) {
      dev::GridOutArgs<T> o{};
      o.src = src; o.F = F; o.ps = nullptr; o.pinv = pinv; o.W = Wd; o.rs = rs; o.cs = cs; o.n = n;
      o.pc = (int)std::min<size_t>(dev::GPANEL, cols.size() - k0);
      for (int p = 0; p < o.pc; ++p) {
        o.col[p] = cols[k0 + p];
        if (factor) {
          const std::complex<double> z = (*factor)[k0 + p];
          if (!(z.real() == 1.0 && z.imag() == 0.0)) { o.scale[p] = taylor_scalar<T>(z); o.scaled |= 1u << p; }
        }
      }
      ProfScope ps(c, EXPV_MI_K_LINCOMB);
      hipLaunchKernelGGL((dev::k_taylor_grid_out<T, 8>), dim3(g_rows), dim3(dev::BLOCK), 0, s, o);
    }
  };

  out_vector(b_dev, from_b, nullptr);
  int p = 0;
  size_t next = 0;
  L.close(b_dev, V[0], eta, -1, 0.0);
  for (int64_t stg = 0; stg < ns; ++stg) {
    GridStagePlan *pl = (next < plans.size() && plans[next].stage == stg) ? &plans[next++] : nullptr;
    const int q = (pl && m > 0) ? (int)pl->interior.size() : 0;
    const int np = (q + dev::GPANEL - 1) / dev::GPANEL;
    const size_t soff = pl ? pl->state_off : 0;
    dev::TaylorGridStage *gs = reinterpret_cast<dev::TaylorGridStage *>(states + soff);
    dev::TaylorGridPanel *pst = reinterpret_cast<dev::TaylorGridPanel *>(states + soff + sizeof(dev::TaylorGridStage));
    std::vector<double> d((size_t)q, 1.0);
    auto coef = [&](int pi) {
      dev::GridCoef<T> co{};
      for (int k = pi * dev::GPANEL; k < std::min(q, (pi + 1) * dev::GPANEL); ++k) co.d[k - pi * dev::GPANEL] = (real_t)d[k];
      return co;
    };
    auto width = [&](int pi) { return panel_width<T>(std::min(dev::GPANEL, q - pi * dev::GPANEL)); };
    for (int j = 1; j <= m; ++j) {
      a.x = V[p]; a.y = V[1 - p]; a.j = j;
      a.c = taylor_scalar<T>(Tt / (double)ns / (double)j);
      for (int k = 0; k < q; ++k) d[k] *= rho[pl->interior[k]];
      ga.G = reinterpret_cast<T *>(panels); ga.ps = pst; ga.gs = gs; ga.co = coef(0);
      with_panel<T>(q > 0 ? width(0) : panel_width<T>(1), [&](auto ptag) {
        constexpr int P = decltype(ptag)::value;
        L.term(ga, a.x, a.y, [](auto fused) { return dev::k_taylor_term_grid<T, P, decltype(fused)::value>; });
      });
      for (int pi = 1; pi < np; ++pi) {
        dev::GridAccumArgs<T> aa{};
        aa.x = a.x; aa.y = a.y; aa.G = reinterpret_cast<T *>(panels + (size_t)pi * pbytes); aa.n = n; aa.co = coef(pi); aa.tol = tc.tol; aa.j = j;
        aa.st = st; aa.ps = pst + pi; aa.gs = gs;
        ProfScope ps(c, EXPV_MI_K_LINCOMB);
        with_panel<T>(width(pi), [&](auto ptag) {
          constexpr int P = decltype(ptag)::value;
          hipLaunchKernelGGL((dev::k_taylor_grid_accum<T, P>), dim3(g_rows), dim3(dev::BLOCK), 0, s, aa);
        });
        ++accum_launches;
      }
      p ^= 1;
    }
    // the interior outputs of the stage: G_k <- exp(mu rho_k h) G_k into W
    for (int pi = 0; pi < np; ++pi) {
      dev::GridOutArgs<T> o{};
      o.src = reinterpret_cast<const T *>(panels + (size_t)pi * pbytes); o.F = F; o.ps = pst + pi; o.pinv = pinv; o.W = Wd; o.rs = rs; o.cs = cs; o.n = n;
      o.pc = std::min(dev::GPANEL, q - pi * dev::GPANEL);
      for (int pp = 0; pp < o.pc; ++pp) {
        const int k = pl->interior[(size_t)pi * dev::GPANEL + pp];
        o.col[pp] = k;
        const std::complex<double> z = std::exp(mu * (rho[k] * h));
        if (!(z.real() == 1.0 && z.imag() == 0.0)) { o.scale[pp] = taylor_scalar<T>(z); o.scaled |= 1u << pp; }
      }
      ProfScope ps(c, EXPV_MI_K_LINCOMB);
      with_panel<T>(width(pi), [&](auto ptag) {
        constexpr int P = decltype(ptag)::value;
        hipLaunchKernelGGL((dev::k_taylor_grid_out<T, P>), dim3(g_rows), dim3(dev::BLOCK), 0, s, o);
      });
    }
    if (pl && m == 0 && !pl->interior.empty()) {      // alpha = 0: exp(mu r_k t) b
      std::vector<std::complex<double>> z;
      for (int k : pl->interior) z.push_back(std::exp(mu * (r[k] * t)));
      out_vector(b_dev, pl->interior, &z);
    }
    L.close(F, V[p], eta, stg, 0.0);
    if (pl) out_vector(F, pl->ends, nullptr);
  }
  HIPCHECK(hipGetLastError());

  // the final state, behind whatever the caller queues after the last output
  hs.assign(sbytes / 8, 0ull);
  before_wait();
  HIPCHECK(hipMemcpyAsync(&hst, st, sizeof(hst), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(hs.data(), states, sbytes, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ++tc.reads;
  taylor_fill_info(tc, hst, info, dinfo);
  if (info) { info[8] = accum_launches; info[9] = qmax; }
  if (col_info) {
    for (int k = 0; k < nt; ++k) { col_info[3 * k] = stage[k]; col_info[3 * k + 1] = 0; col_info[3 * k + 2] = kind[k]; }
    for (const auto &pl : plans) {
      const char *sp = reinterpret_cast<const char *>(hs.data()) + pl.state_off;
      dev::TaylorGridStage gs;
      std::memcpy(&gs, sp, sizeof(gs));
      for (int k : pl.ends) col_info[3 * k + 1] = (int64_t)gs.fterms;
      for (size_t e = 0; m > 0 && e < pl.interior.size(); ++e) {
        dev::TaylorGridPanel ps;
        std::memcpy(&ps, sp + sizeof(gs) + sizeof(ps) * (e / dev::GPANEL), sizeof(ps));
        col_info[3 * pl.interior[e] + 1] = (int64_t)ps.terms[e % dev::GPANEL];
      }
    }
  }
}

}  // namespace

void taylor_grid_run(Ctx *c, Op &op, double t_re, double t_im, const double *r, int nt, const void *b_dev, void *W, int64_t ldw, int w_layout,
                     int w_loc, int precision, int64_t max_matvecs, double opnorm, int64_t info[10], double dinfo[4], int64_t *col_info) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  const size_t esz = dtype_size(op.dtype);
  const bool colmajor = w_layout == EXPV_MI_BLOCK_COL_MAJOR;
  DevBuf wstage;
  try {
    void *Wd = W;
    int64_t ld = ldw;
    if (w_loc == EXPV_MI_HOST) {      // a compact device copy of the same layout, copied out before the one wait
      ld = colmajor ? n : (int64_t)nt;
      wstage.take_from(c, (size_t)n * (size_t)nt * esz + 16);
      Wd = wstage.p;
    }
    const std::function<void()> before_wait = [&] {
      if (w_loc == EXPV_MI_HOST) taylor_block_copy_host(s, W, ldw, wstage.p, ld, w_layout, n, nt, esz, hipMemcpyDeviceToHost);
    };
    dispatch_dtype(op.dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      grid_run_T<T>(c, op, std::complex<double>(t_re, t_im), r, nt, reinterpret_cast<const T *>(b_dev), reinterpret_cast<T *>(Wd), colmajor ? 1 : ld,
                    colmajor ? ld : 1, precision, max_matvecs, opnorm, before_wait, info, dinfo, col_info);
    });
  } catch (...) {
    (void)hipStreamSynchronize(s);      // (the staging copy of W goes back to the context: nothing may still be writing it)
    throw;
  }
}

}  // namespace expv_mi
