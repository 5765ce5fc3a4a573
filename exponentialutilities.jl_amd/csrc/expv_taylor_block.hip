// expv_taylor_block.hip -- exp(tA)B for an n x p block by the truncated Taylor series of expv_taylor.hip: p independent problems
// that share every pass over the operator (Al-Mohy & Higham wrote the algorithm for a block; SIAM J. Sci. Comput. 33, 2011).
//
// (mu, alpha, m*, s) depend on A and t alone and are computed once (taylor_shift_plan).  Columns run in panels of P in {2, 4, 8} on
// three INTERLEAVED work vectors [row][P] (v ping, v pong, F): a term launch reads the operator once for the whole panel, and the
// gather of a column index is one aligned P * sizeof(T) access.  Every column keeps its own stopping state -- maxima, c1, counters
// as arrays of words, stopped / ended / NaN as bit masks -- in one state block per panel; a column that has stopped or ended is
// masked (F written back unchanged, no maxima) until the stage's closing launch rebuilds its v.  The arithmetic of a column is the
// single call's by construction: acc summed over the slots / diagonals in ascending order, then the element step the single kernel
// calls too (taylor_step, taylor_state.h) -- so column k of the result is bit for bit what expv_mi_expv_taylor returns for column k of B.
// The operator view, the fused predicate and the bookkeeping of a term launch are those of taylor_term.h.
//
// Synchronisation is that of expv_taylor.hip: agent-scope atomic maxima / OR, one ticket per launch, lane 0 of the last workgroup
// to arrive runs the P tests and re-arms the state through L1-bypassing accesses.
//
// Operators without a fused form (SELL with overflow entries, dense, matrix-free) and a block of one column run the single-vector
// loop (taylor_run) column by column behind the one shared plan.
#include <cmath>
#include <complex>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#include "engine.h"
#include "kernel_common.h"
#include "taylor_state.h"
#include "taylor_term.h"

namespace expv_mi {
namespace dev {

constexpr int PANEL = 8;      // columns of a full panel; a remainder runs in the smallest P in {2, 4, 8} that holds it

// Slots / diagonals a lane keeps in flight: one of them is 16 P bytes of gathered operands (4 P registers) beside 16 P bytes each
// of accumulators, x_i and F.  Chosen from the register counts the compiler reports: no spills, and at
// least two waves per SIMD at P = 8.
template <int P> struct InFlight { static constexpr int Q = P <= 4 ? 4 : 2; };

// Stage state of one panel, 64 words of 8 bytes; the access rules are those of TaylorState.
struct TaylorBlockState {
  unsigned long long maxv[PANEL], maxf[PANEL];      // running maxima of |v_ik| and |F_ik| per column
  unsigned long long c1[PANEL], fnorm[PANEL];
  unsigned long long apps[PANEL], early[PANEL], nf_stage[PANEL];
  unsigned long long nanv, nanf;                    // bit k: a NaN among v / F of column k
  unsigned long long ticket;
  unsigned long long stopped, ended;                // bit k: column k (padding columns are zero: stopped from the start)
  unsigned long long worked;                        // term launches that did not return at once
  unsigned long long spare[2];
};
static_assert(sizeof(TaylorBlockState) == 512, "TaylorBlockState layout");

// (RowP, one row of an interleaved work vector, and BlockColumns, the right-hand side of the operator loops for P columns: sparse_rows.h)

// taylor_arrive for P columns: this workgroup's maxima into the panel's state, then one ticket
template <int P>
__device__ __forceinline__ bool block_arrive(TaylorBlockState *st, double (&mv)[P], double (&mf)[P], unsigned nanv, unsigned nanf) {
  __shared__ double m_s[BLOCK / 64][2 * P];
  __shared__ unsigned nan_s[BLOCK / 64][2];
  __shared__ int last_s;
  unsigned wv = 0u, wf = 0u;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    mv[p] = wave_max(mv[p]);
    mf[p] = wave_max(mf[p]);
    wv |= __any((int)((nanv >> p) & 1u)) ? (1u << p) : 0u;
    wf |= __any((int)((nanf >> p) & 1u)) ? (1u << p) : 0u;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int p = 0; p < P; ++p) { m_s[wave][p] = mv[p]; m_s[wave][P + p] = mf[p]; }
    nan_s[wave][0] = wv;
    nan_s[wave][1] = wf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) {
#pragma unroll
      for (int p = 0; p < P; ++p) { mv[p] = fmax(mv[p], m_s[w][p]); mf[p] = fmax(mf[p], m_s[w][P + p]); }
      wv |= nan_s[w][0];
      wf |= nan_s[w][1];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (mv[p] > 0.0) atomicMax(&st->maxv[p], (unsigned long long)__double_as_longlong(mv[p]));
      if (mf[p] > 0.0) atomicMax(&st->maxf[p], (unsigned long long)__double_as_longlong(mf[p]));
    }
    if (wv) atomicOr(&st->nanv, (unsigned long long)wv);
    if (wf) atomicOr(&st->nanf, (unsigned long long)wf);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __hip_atomic_fetch_add(&st->ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = (t == (unsigned long long)gridDim.x - 1ull);
  }
  __syncthreads();
  return last_s != 0;
}
template <int P>
__device__ __forceinline__ void block_rearm(TaylorBlockState *st) {
#pragma unroll
  for (int p = 0; p < P; ++p) { ts_store(&st->maxv[p], 0ull); ts_store(&st->maxf[p], 0ull); }
  ts_store(&st->nanv, 0ull);
  ts_store(&st->nanf, 0ull);
  ts_store(&st->ticket, 0ull);
}
__device__ __forceinline__ unsigned block_mask(const unsigned long long *a, const unsigned long long *b) {      // wave-uniform
  return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(ts_load(a) | (b ? ts_load(b) : 0ull)));
}

template <class T>
struct BlockTermArgs {
  TaylorOpView<T> op;
  const T *x;                                     // v of the previous term, [row][P]
  T *y, *F;
  int64_t n;
  T c, mu;                                        // (t / s) / j and tr(A) / n
  double tol;
  int j, m;
  TaylorBlockState *st;
};

// k_taylor_term<T, true> for P columns: the lane <-> row mapping is the same (one 16-byte row pack of the operator per lane), the
// operator's values and column indices are loaded once and used P times
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_taylor_term_block(BlockTermArgs<T> a) {
  constexpr unsigned ALL = (1u << P) - 1u;
  const unsigned off = block_mask(&a.st->stopped, &a.st->ended) & ALL;
  if (off == ALL) return;
  constexpr int N = Pack<T>::N;
  constexpr int SH = 64 * N;
  using Row = RowP<T, P>;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t nsl = (a.n + SH - 1) / SH;
  double mv[P], mf[P];
#pragma unroll
  for (int p = 0; p < P; ++p) mv[p] = mf[p] = 0.0;
  unsigned nanv = 0u, nanf = 0u;
  for (int64_t slice = (int64_t)blockIdx.x * (BLOCK / 64) + wave; slice < nsl; slice += (int64_t)gridDim.x * (BLOCK / 64)) {
    const int64_t i = slice * SH + (int64_t)lane * N;      // (the work vectors are padded to whole slices: no tail path)
    T acc[N][P];
    BlockColumns<T, P> xs{a.x, acc};
    if (a.op.ndiag > 0) dia_walk<T, InFlight<P>::Q>(a.op.dia_val, a.op.dia_ld, a.op.ndiag, a.op.dia_off, i, a.n, xs);
    else sell_walk<T, InFlight<P>::Q>(a.op.A, slice, lane, xs);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const Row xi = *reinterpret_cast<const Row *>(a.x + (i + k) * P);
      Row f = *reinterpret_cast<const Row *>(a.F + (i + k) * P);
      Row y;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        T v, fn;
        taylor_step(acc[k][p], a.mu, xi.v[p], a.c, f.v[p], v, fn);
        y.v[p] = v;
        const bool live = !((off >> p) & 1u);      // (a masked column: F as it was, no maxima; its v is rebuilt when the stage closes)
        if (live) f.v[p] = fn;
        if (live && i + k < a.n) {
          note_abs(abs_T(v), mv[p], nanv, 1u << p);
          note_abs(abs_T(fn), mf[p], nanf, 1u << p);
        }
      }
      *reinterpret_cast<Row *>(a.y + (i + k) * P) = y;
      *reinterpret_cast<Row *>(a.F + (i + k) * P) = f;
    }
  }
  if (block_arrive<P>(a.st, mv, mf, nanv, nanf) && threadIdx.x == 0) {      // the test of taylor_term_test, column by column
    TaylorBlockState *st = a.st;
    const unsigned long long nv = ts_load(&st->nanv), nf = ts_load(&st->nanf);
    unsigned long long stopped = ts_load(&st->stopped);
    for (int p = 0; p < P; ++p) {
      if ((off >> p) & 1u) continue;
      const double c2 = ((nv >> p) & 1ull) ? taylor_qnan() : ts_loadf(&st->maxv[p]);
      const double fn = ((nf >> p) & 1ull) ? taylor_qnan() : ts_loadf(&st->maxf[p]);
      const double c1 = ts_loadf(&st->c1[p]);
      ts_store(&st->apps[p], ts_load(&st->apps[p]) + 1ull);
      if (c1 + c2 <= a.tol * fn) {
        stopped |= 1ull << p;
        if (a.j < a.m) ts_store(&st->early[p], ts_load(&st->early[p]) + 1ull);
      } else {
        ts_storef(&st->c1[p], c2);
      }
    }
    ts_store(&st->stopped, stopped);
    ts_store(&st->worked, ts_load(&st->worked) + 1ull);
    block_rearm<P>(st);
  }
}

// lane 0 of the last workgroup of a closing launch (k_taylor_close), for the columns in `cols`; stage < 0: no finite test
template <int P>
__device__ __forceinline__ void block_close_test(TaylorBlockState *st, unsigned cols, int stage, int more) {
  const unsigned long long nf = ts_load(&st->nanf);
  unsigned long long stopped = ts_load(&st->stopped), ended = ts_load(&st->ended);
  for (int p = 0; p < P; ++p) {
    if (!((cols >> p) & 1u)) continue;
    const double fn = ((nf >> p) & 1ull) ? taylor_qnan() : ts_loadf(&st->maxf[p]);
    ts_storef(&st->c1[p], fn);
    ts_storef(&st->fnorm[p], fn);
    const bool finite = fn < __longlong_as_double(0x7ff0000000000000ll);
    if (stage >= 0 && !finite) {
      ended |= 1ull << p;
      ts_store(&st->nf_stage[p], (unsigned long long)stage + 1ull);
    }
    const bool zero = fn == 0.0;      // a zero column stays zero: the stage that follows applies nothing to it
    stopped = zero ? (stopped | (1ull << p)) : (stopped & ~(1ull << p));
    if (zero && more) ts_store(&st->early[p], ts_load(&st->early[p]) + 1ull);
  }
  ts_store(&st->stopped, stopped);
  ts_store(&st->ended, ended);
  block_rearm<P>(st);
}

// Closes a stage for every column that has not ended: F = eta F (scale != 0), v = F, c1 = |F|_inf, the finite test, the state of
// the next stage.  An ended column is left alone.
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_taylor_close_block(T *F, T *v, int64_t n, T eta, int scale, int stage, int more, TaylorBlockState *st) {
  constexpr unsigned ALL = (1u << P) - 1u;
  const unsigned ended = block_mask(&st->ended, nullptr) & ALL;
  if (ended == ALL) return;
  using Row = RowP<T, P>;
  double mv[P], mf[P];
#pragma unroll
  for (int p = 0; p < P; ++p) mv[p] = mf[p] = 0.0;
  unsigned nanf = 0u;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * BLOCK) {
    Row f = *reinterpret_cast<const Row *>(F + r * P);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if ((ended >> p) & 1u) continue;
      if (scale) f.v[p] = mul_as_single(eta, f.v[p]);
      note_abs(abs_T(f.v[p]), mf[p], nanf, 1u << p);
    }
    if (scale) *reinterpret_cast<Row *>(F + r * P) = f;
    *reinterpret_cast<Row *>(v + r * P) = f;
  }
  if (block_arrive<P>(st, mv, mf, 0u, nanf) && threadIdx.x == 0) block_close_test<P>(st, ~ended & ALL, stage, more);
}

// Pack-in: columns [0, pc) of the caller's block (element (i, k) at B[i * rs + k * cs]; row p[i] of it for a reordered operator)
// into F and v, padding columns and padding rows zero -- and the first closing launch of the panel (src = b, no scaling, stage -1).
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_taylor_block_in(const T *__restrict__ B, int64_t rs, int64_t cs, int pc, const int32_t *__restrict__ perm,
                                                           T *F, T *v, int64_t n, int64_t rows, TaylorBlockState *st) {
  constexpr unsigned ALL = (1u << P) - 1u;
  using Row = RowP<T, P>;
  double mv[P], mf[P];
#pragma unroll
  for (int p = 0; p < P; ++p) mv[p] = mf[p] = 0.0;
  unsigned nanf = 0u;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < rows; r += (int64_t)gridDim.x * BLOCK) {
    Row f;
    const int64_t src = (r < n) ? (perm ? (int64_t)perm[r] : r) : 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      f.v[p] = (r < n && p < pc) ? B[src * rs + (int64_t)p * cs] : ST<T>::zero();
      note_abs(abs_T(f.v[p]), mf[p], nanf, 1u << p);
    }
    *reinterpret_cast<Row *>(F + r * P) = f;
    *reinterpret_cast<Row *>(v + r * P) = f;
  }
  if (block_arrive<P>(st, mv, mf, 0u, nanf) && threadIdx.x == 0) block_close_test<P>(st, ALL, -1, 1);
}

// Pack-out: W(i, k) = F[row of i][k] for the pc columns of the panel, rows back in the caller's ordering
template <class T, int P>
__global__ __launch_bounds__(BLOCK) void k_taylor_block_out(const T *__restrict__ F, const int32_t *__restrict__ pinv, T *__restrict__ W, int64_t rs,
                                                            int64_t cs, int pc, int64_t n) {
  using Row = RowP<T, P>;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * BLOCK) {
    const Row f = *reinterpret_cast<const Row *>(F + (pinv ? (int64_t)pinv[r] : r) * P);
#pragma unroll
    for (int p = 0; p < P; ++p)
      if (p < pc) W[r * rs + (int64_t)p * cs] = f.v[p];
  }
}

// column blockIdx.y of a block between two layouts: dst(i, k) = src(idx ? idx[i] : i, k)   (the column-by-column path)
template <class T>
__global__ __launch_bounds__(BLOCK) void k_taylor_block_copy(const T *__restrict__ src, int64_t srs, int64_t scs, T *__restrict__ dst, int64_t drs,
                                                             int64_t dcs, const int32_t *__restrict__ idx, int64_t n) {
  const int64_t k = blockIdx.y;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * BLOCK)
    dst[r * drs + k * dcs] = src[(idx ? (int64_t)idx[r] : r) * srs + k * scs];
}

}  // namespace dev

namespace {

struct BlockView {      // element (i, k) at p[i * rs + k * cs]
  char *p;
  int64_t rs, cs;
};
BlockView view_of(const void *p, int layout, int64_t ld) {
  return layout == EXPV_MI_BLOCK_COL_MAJOR ? BlockView{(char *)p, 1, ld} : BlockView{(char *)p, ld, 1};
}
// a host block <-> its compact device copy of the same layout (the elements between columns / rows of a padded ld stay out of it)
void copy_block(hipStream_t s, void *dst, int64_t ld_dst, const void *src, int64_t ld_src, int layout, int64_t n, int ncols, size_t esz,
                hipMemcpyKind kind) {
  const size_t width = (size_t)(layout == EXPV_MI_BLOCK_COL_MAJOR ? n : (int64_t)ncols) * esz;
  const size_t height = (size_t)(layout == EXPV_MI_BLOCK_COL_MAJOR ? (int64_t)ncols : n);
  if (ld_dst == ld_src && (size_t)ld_src * esz == width) HIPCHECK(hipMemcpyAsync(dst, src, width * height, kind, s));
  else HIPCHECK(hipMemcpy2DAsync(dst, (size_t)ld_dst * esz, src, (size_t)ld_src * esz, width, height, kind, s));
}

struct BlockResult {      // what the two paths hand back per column
  std::vector<int64_t> apps, early, nf;
  std::vector<double> normF;
  int64_t worked = 0;
};

// the panels of the block kernel; Bv / Wv are device views
template <class T>
void run_panels(Ctx *c, Op &op, std::complex<double> t, BlockView Bv, BlockView Wv, int ncols, TaylorCall &tc, DevBuf &work, BlockResult &res,
                const std::function<void()> &before_wait) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  constexpr int N = dev::Pack<T>::N, SH = 64 * N;
  constexpr int PMIN = (16 / (int)sizeof(T)) > 2 ? 16 / (int)sizeof(T) : 2;      // a row of the work vectors is at least one 16-byte pack
  const int64_t nsl = (n + SH - 1) / SH, rows = nsl * SH;
  const int npanels = (ncols + dev::PANEL - 1) / dev::PANEL;
  const size_t vbytes = (size_t)rows * dev::PANEL * sizeof(T), sbytes = sizeof(dev::TaylorBlockState) * (size_t)npanels;
  work.take_from(c, sbytes + 3 * vbytes);
  char *base = work.as<char>();
  dev::TaylorBlockState *states = reinterpret_cast<dev::TaylorBlockState *>(base);
  T *V[2] = {reinterpret_cast<T *>(base + sbytes), reinterpret_cast<T *>(base + sbytes + vbytes)};
  T *F = reinterpret_cast<T *>(base + sbytes + 2 * vbytes);
  HIPCHECK(hipMemsetAsync(states, 0, sbytes, s));

  const std::complex<double> mu(tc.mu_re, tc.mu_im);
  const int m = tc.m;
  const int64_t ns = tc.s;
  dev::BlockTermArgs<T> a{};
  a.op = taylor_op_view<T>(c, op);
  a.F = F; a.n = n; a.mu = taylor_scalar<T>(mu); a.tol = tc.tol; a.m = m;
  const int g_term = dev::taylor_grid(nsl, dev::BLOCK / 64), g_rows = dev::taylor_grid(rows, dev::BLOCK);
  const std::complex<double> eta = taylor_stage_factor(mu, t, ns);
  const bool scale = !(eta.real() == 1.0 && eta.imag() == 0.0);
  const int32_t *perm = op.perm ? op.perm->p.as<int32_t>() : nullptr, *pinv = op.perm ? op.perm->pinv.as<int32_t>() : nullptr;

  auto panel = [&](auto ptag, int col0, int pc, dev::TaylorBlockState *st) {
    constexpr int P = decltype(ptag)::value;
    const T *Bp = reinterpret_cast<const T *>(Bv.p) + (int64_t)col0 * Bv.cs;
    T *Wp = reinterpret_cast<T *>(Wv.p) + (int64_t)col0 * Wv.cs;
    a.st = st;
    {
      ProfScope ps(c, EXPV_MI_K_LINCOMB);
      hipLaunchKernelGGL((dev::k_taylor_block_in<T, P>), dim3(g_rows), dim3(dev::BLOCK), 0, s, Bp, Bv.rs, Bv.cs, pc, perm, F, V[0], n, rows, st);
    }
    int p = 0;
    for (int64_t stage = 0; stage < ns; ++stage) {
      for (int j = 1; j <= m; ++j) {
        a.x = V[p]; a.y = V[1 - p]; a.j = j;
        a.c = taylor_scalar<T>(t / (double)ns / (double)j);
        taylor_term_launch(c, op, tc, true, a.x, a.y,
                           [&] { hipLaunchKernelGGL((dev::k_taylor_term_block<T, P>), dim3(g_term), dim3(dev::BLOCK), 0, s, a); });
        p ^= 1;
      }
      ProfScope ps(c, EXPV_MI_K_LINCOMB);
      hipLaunchKernelGGL((dev::k_taylor_close_block<T, P>), dim3(g_rows), dim3(dev::BLOCK), 0, s, F, V[p], n, taylor_scalar<T>(eta), scale ? 1 : 0,
                         (int)std::min<int64_t>(stage, 2147483646), (int)(stage + 1 < ns), st);
    }
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL((dev::k_taylor_block_out<T, P>), dim3(g_rows), dim3(dev::BLOCK), 0, s, F, pinv, Wp, Wv.rs, Wv.cs, pc, n);
  };
  for (int q = 0; q < npanels; ++q) {
    const int col0 = q * dev::PANEL, pc = std::min(dev::PANEL, ncols - col0);
    const int P = std::max(PMIN, pc <= 2 ? 2 : pc <= 4 ? 4 : 8);
    if constexpr (PMIN <= 2) {
      if (P == 2) { panel(std::integral_constant<int, 2>(), col0, pc, states + q); continue; }
    }
    if (P == 4) panel(std::integral_constant<int, 4>(), col0, pc, states + q);
    else panel(std::integral_constant<int, 8>(), col0, pc, states + q);
  }
  HIPCHECK(hipGetLastError());

  // the state read-back shares the wait of whatever the caller queues behind the last pack-out
  std::vector<dev::TaylorBlockState> h((size_t)npanels);
  before_wait();
  HIPCHECK(hipMemcpyAsync(h.data(), states, sbytes, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ++tc.reads;
  for (int k = 0; k < ncols; ++k) {
    const dev::TaylorBlockState &st = h[(size_t)(k / dev::PANEL)];
    const int p = k % dev::PANEL;
    res.apps[k] = (int64_t)st.apps[p]; res.early[k] = (int64_t)st.early[p]; res.nf[k] = (int64_t)st.nf_stage[p];
    res.normF[k] = f64_of(st.fnorm[p]);
  }
  for (const auto &st : h) res.worked += (int64_t)st.worked;
}

// column by column through the single-vector loop, behind the shared plan
void run_columns(Ctx *c, Op &op, double t_re, double t_im, BlockView Bv, BlockView Wv, int ncols, TaylorCall &tc, DevBuf &work, BlockResult &res,
                 const std::function<void()> &before_wait) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  const size_t esz = dtype_size(op.dtype), vbytes = up16((size_t)n * esz) + 16, sbytes = sizeof(dev::TaylorState) * (size_t)ncols;
  const int64_t ldx = (int64_t)(up16((size_t)n * esz) / esz);
  work.take_from(c, sbytes + 2 * vbytes + (size_t)ncols * (size_t)ldx * esz + 16);
  char *base = work.as<char>();
  char *X = base + sbytes + 2 * vbytes;
  HIPCHECK(hipMemsetAsync(base, 0, sbytes, s));
  const int32_t *perm = op.perm ? op.perm->p.as<int32_t>() : nullptr, *pinv = op.perm ? op.perm->pinv.as<int32_t>() : nullptr;
  auto copy = [&](BlockView from, BlockView to, const int32_t *idx) { taylor_block_copy(c, op, from.p, from.rs, from.cs, to.p, to.rs, to.cs, idx, ncols); };
  const BlockView Xv{X, 1, ldx};
  copy(Bv, Xv, perm);
  for (int k = 0; k < ncols; ++k) {
    char *xk = X + (size_t)k * (size_t)ldx * esz;      // b on entry, F of the column afterwards
    taylor_run(c, op, t_re, t_im, xk, base + sizeof(dev::TaylorState) * (size_t)k, base + sbytes, base + sbytes + vbytes, xk, tc);
  }
  copy(Xv, Wv, pinv);
  HIPCHECK(hipGetLastError());
  std::vector<dev::TaylorState> h((size_t)ncols);
  before_wait();
  HIPCHECK(hipMemcpyAsync(h.data(), base, sbytes, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ++tc.reads;
  for (int k = 0; k < ncols; ++k) {
    res.apps[k] = (int64_t)h[k].apps; res.early[k] = (int64_t)h[k].early; res.nf[k] = (int64_t)h[k].nf_stage;
    res.normF[k] = f64_of(h[k].fnorm);
    res.worked += (int64_t)h[k].apps;      // (a term launch of the single-vector loop that did work is an application)
  }
}

}  // namespace

void taylor_block_copy_host(hipStream_t s, void *dst, int64_t ld_dst, const void *src, int64_t ld_src, int layout, int64_t n, int ncols, size_t esz,
                            hipMemcpyKind kind) {
  copy_block(s, dst, ld_dst, src, ld_src, layout, n, ncols, esz, kind);
}

void taylor_block_copy(Ctx *c, Op &op, const void *src, int64_t srs, int64_t scs, void *dst, int64_t drs, int64_t dcs, const int32_t *idx, int ncols) {
  ProfScope ps(c, EXPV_MI_K_LINCOMB);
  const int64_t n = op.n;
  dispatch_dtype(op.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    for (int k0 = 0; k0 < ncols; k0 += 65535) {      // (gridDim.y <= 65535)
      const dim3 g((unsigned)dev::taylor_grid(n, dev::BLOCK), (unsigned)std::min(ncols - k0, 65535));
      hipLaunchKernelGGL(dev::k_taylor_block_copy<T>, g, dim3(dev::BLOCK), 0, c->stream, reinterpret_cast<const T *>(src) + (int64_t)k0 * scs, srs, scs,
                         reinterpret_cast<T *>(dst) + (int64_t)k0 * dcs, drs, dcs, idx, n);
    }
  });
}

void taylor_block_run(Ctx *c, Op &op, double t_re, double t_im, const void *B, int64_t ldb, int ncols, int b_layout, int b_loc, void *W,
                      int64_t ldw, int w_layout, int w_loc, int precision, int64_t max_matvecs, double opnorm, int64_t info[8],
                      double dinfo[4], int64_t *col_info, double *col_normF) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  const size_t esz = dtype_size(op.dtype);
  TaylorCall tc;
  DevBuf head, work, bstage, wstage;
  BlockResult res;
  res.apps.assign((size_t)ncols, 0); res.early.assign((size_t)ncols, 0); res.nf.assign((size_t)ncols, 0); res.normF.assign((size_t)ncols, 0.0);
  try {
    head.take_from(c, taylor_head_bytes());
    taylor_shift_plan(c, op, t_re, t_im, precision, max_matvecs, opnorm, head.p, tc);      // (a refusal: nothing has touched W)
    const int64_t ld_compact[2] = {n, (int64_t)ncols};
    BlockView Bv = view_of(B, b_layout, ldb), Wv = view_of(W, w_layout, ldw);
    if (b_loc == EXPV_MI_HOST) {
      bstage.take_from(c, (size_t)n * (size_t)ncols * esz + 16);
      copy_block(s, bstage.p, ld_compact[b_layout], B, ldb, b_layout, n, ncols, esz, hipMemcpyHostToDevice);
      Bv = view_of(bstage.p, b_layout, ld_compact[b_layout]);
    }
    if (w_loc == EXPV_MI_HOST) {
      wstage.take_from(c, (size_t)n * (size_t)ncols * esz + 16);
      Wv = view_of(wstage.p, w_layout, ld_compact[w_layout]);
    }
    const std::function<void()> before_wait = [&] {
      if (w_loc == EXPV_MI_HOST) copy_block(s, W, ldw, wstage.p, ld_compact[w_layout], w_layout, n, ncols, esz, hipMemcpyDeviceToHost);
    };
    if (taylor_fused(op) && ncols >= 2) {
      tc.path = 1;
      dispatch_dtype(op.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        run_panels<T>(c, op, std::complex<double>(t_re, t_im), Bv, Wv, ncols, tc, work, res, before_wait);
      });
    } else {
      run_columns(c, op, t_re, t_im, Bv, Wv, ncols, tc, work, res, before_wait);      // (sets tc.path: 1 only for one column of a fused operator)
    }
  } catch (...) {
    (void)hipStreamSynchronize(s);      // (the work vectors go back to the context: nothing may still be writing them)
    throw;
  }
  int64_t apps = 0, bad = 0;
  double fmaxn = 0.0;
  for (int k = 0; k < ncols; ++k) {
    apps += res.apps[k];
    bad += res.nf[k] != 0;
    if (res.normF[k] != res.normF[k] || fmaxn != fmaxn) fmaxn = std::numeric_limits<double>::quiet_NaN();
    else fmaxn = std::max(fmaxn, res.normF[k]);
    if (col_info) { col_info[3 * k] = res.apps[k]; col_info[3 * k + 1] = res.early[k]; col_info[3 * k + 2] = res.nf[k]; }
    if (col_normF) col_normF[k] = res.normF[k];
  }
  if (info) {
    info[0] = tc.m; info[1] = tc.s; info[2] = apps; info[3] = res.worked; info[4] = tc.launches; info[5] = tc.reads; info[6] = tc.path;
    info[7] = bad;
  }
  if (dinfo) { dinfo[0] = tc.alpha; dinfo[1] = tc.mu_re; dinfo[2] = tc.mu_im; dinfo[3] = fmaxn; }
}

}  // namespace expv_mi
