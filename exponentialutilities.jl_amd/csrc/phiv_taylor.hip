// phiv_taylor.hip -- w = phi_0(tA) u_0 + t phi_1(tA) u_1 + ... + t^p phi_p(tA) u_p without a Krylov basis: the truncated Taylor series
// of expv_taylor.hip on the augmented matrix of Al-Mohy & Higham (SIAM J. Sci. Comput. 33, 2011, Theorem 2.1 and section 5)
//
//   A~ = [A W; 0 J],  W = [u_p, ..., u_1],  J the p x p upward shift:   the first n rows of exp(t A~) [u_0; e_p]  =  sum_k t^k phi_k(tA) u_k
//
// A~ is never formed and no vector has n + p rows.  The p tail components of every term do not depend on the data: at stage start
// they are zeta_0 = exp(tau J) e_p (tau = stage h, h = t / s), and term j maps them to zeta_j = (h / j)(J - mu I) zeta_{j-1}; the sum of
// the zeta_j times exp(mu h) is exp(h J) zeta_0, the next stage's start, exactly.  The host computes them in (complex) double, and
// the device adds what they send into the n head rows:
//
//   v_j[i] = c_j ((A v_{j-1})[i] - mu v_{j-1}[i]) + sum_{k=1..p} g_j[p+1-k] u_k[i],   g_j = c_j zeta_{j-1},  c_j = h / j,   F += v_j
//
// The stopping test is expv_taylor's with the tail as a floor: c2 = max(|v_j|_inf, |zeta_j|_inf U), c1 at stage start
// max(|F|_inf, |zeta_0|_inf U), U = max |u_k[i]| over k >= 1 -- without it a call whose u_0 is zero would stop on its first, zero,
// terms.  The norm behind (m*, s) is that of diag(I, nu) A~ diag(I, 1 / nu) - mu I with nu = 2^-ceil(log2 max_i sum_{k>=1} |u_k[i]|)
// (the paper's scaling against over-scaling: the similarity changes nothing but the norm), mu = tr(A) / (n + p).
//
// One column (p = 0) is exp(tA) u_0: it runs the single-vector loop of expv_taylor.hip itself, plan included.  With p >= 1 the term
// kernel k_phiv_term below has loops of its own on the shared element arithmetic; the host side is TaylorLaunch (taylor_term.h).
#include <cmath>
#include <complex>
#include <cstring>
#include <limits>

#include "engine.h"
#include "kernel_common.h"
#include "taylor_state.h"
#include "taylor_term.h"

namespace expv_mi {

constexpr int PHIV_TAYLOR_PMAX = 8;      // p <= 8: a lane of the fused term keeps one 16-byte pack of every column in flight
int phiv_taylor_pmax() { return PHIV_TAYLOR_PMAX; }

// nu = 2^-ceil(log2 w) (1 for w = 0 and for a w that is not finite: alpha is not finite then either, and the call is refused)
__host__ __device__ static inline double phiv_nu(double w) {
  if (!(w > 0.0) || !(w < std::numeric_limits<double>::infinity())) return 1.0;
  int e;
  const double f = frexp(w, &e);      // w = f 2^e, 0.5 <= f < 1
  return ldexp(1.0, -(f == 0.5 ? e - 1 : e));
}

namespace dev {

template <class T>
struct PhivTermArgs {
  TaylorTermArgs<T> t;
  const T *B;                     // column-major, column k (= u_k) at B + k ldb; column 0 is not read by a term
  int64_t ldb;
  T g[PHIV_TAYLOR_PMAX];          // g[k - 1]: the coefficient of u_k in this term, rounded to T
  unsigned mask;                  // bit k - 1: g[k - 1] != 0 (0: the launch does not touch B)
  double tail;                    // |zeta_j|_inf U
};

// the columns this term needs, one 16-byte pack each (the last pack of a column element-wise, as every caller vector)
template <class T>
__device__ __forceinline__ void phiv_load(const PhivTermArgs<T> &a, int64_t i, Pack<T> (&u)[PHIV_TAYLOR_PMAX]) {
#pragma unroll
  for (int k = 0; k < PHIV_TAYLOR_PMAX; ++k) {
    if ((a.mask >> k) & 1u) {      // (uniform: a kernel argument)
      const T *col = a.B + (int64_t)(k + 1) * a.ldb;
      u[k] = ld_pack_user(col, i, a.t.n, is_al16(col));
    }
  }
}
template <class T>
__device__ __forceinline__ void phiv_add(const PhivTermArgs<T> &a, const Pack<T> (&u)[PHIV_TAYLOR_PMAX], int r, T &y) {
#pragma unroll
  for (int k = 0; k < PHIV_TAYLOR_PMAX; ++k)
    if ((a.mask >> k) & 1u) ST<T>::fma_(y, a.g[k], u[k].v[r]);
}

// k_taylor_term + the rank-p add: y_i = c ((A x)_i - mu x_i) + sum_k g_k u_k[i], F_i += y_i, maxima, ticket, and the test with the
// tail as a floor.  The packs of the needed columns are issued with the x_i and F loads, ahead of the operator's slots.
// The roundings: y = c v by the first half of the element step (taylor_product, taylor_state.h), then one fused multiply-add chain
// per needed column in ascending k, then the PLAIN sum F + y for every element type -- also when the mask is empty: a term of phiv
// never fuses c v into F as the real exp(tA)b step does.
// This kernel does NOT go through taylor_sweep (taylor_term.h): it keeps the scalar registers short (g, the column alignments and
// the mask bits live there), and with its rows or even one element behind a function of its own the compiler spills 2 .. 6 more of
// them (its resource report; profiles/taylor_term_regs.txt).  So the two loops stand here as text, on the shared small pieces.
template <class T, bool FUSED>
__global__ __launch_bounds__(BLOCK) void k_phiv_term(PhivTermArgs<T> pa) {
  const TaylorTermArgs<T> &a = pa.t;
  if (taylor_skip(a.st)) return;
  constexpr int N = Pack<T>::N;
  const bool alx = is_al16(a.x), aly = is_al16(a.y), alf = is_al16(a.F);
  double mv = 0.0, mf = 0.0;
  unsigned nan = 0u;
  if constexpr (FUSED) {
    constexpr int SH = 64 * N;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nsl = (a.n + SH - 1) / SH;
    for (int64_t slice = (int64_t)blockIdx.x * (BLOCK / 64) + wave; slice < nsl; slice += (int64_t)gridDim.x * (BLOCK / 64)) {
      const int64_t i = slice * SH + (int64_t)lane * N;
      const Pack<T> xi = ld_pack_user(a.x, i, a.n, alx);
      Pack<T> f = ld_pack_user(a.F, i, a.n, alf);
      Pack<T> u[PHIV_TAYLOR_PMAX];
      if (pa.mask) phiv_load<T>(pa, i, u);
      Pack<T> acc;
      if (a.op.ndiag > 0) dia_rows<T>(a.op.dia_val, a.op.dia_ld, a.op.ndiag, a.op.dia_off, i, a.n, a.x, acc.v);
      else sell_rows<T>(a.op.A, slice, lane, a.x, acc.v);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        T v, y;
        taylor_product(acc.v[k], a.mu, xi.v[k], a.c, v, y);
        if (pa.mask) phiv_add<T>(pa, u, k, y);
        acc.v[k] = y;
        f.v[k] = add_as_written(f.v[k], y);
        if (i + k < a.n) {
          note_abs(abs_T(y), mv, nan, 1u);
          note_abs(abs_T(f.v[k]), mf, nan, 2u);
        }
      }
      st_pack_user(a.y, i, a.n, aly, acc);
      st_pack_user(a.F, i, a.n, alf, f);
    }
  } else {
    for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * N; i < a.n; i += (int64_t)gridDim.x * BLOCK * N) {
      const Pack<T> xi = ld_pack_user(a.x, i, a.n, alx);
      Pack<T> acc = ld_pack_user(a.y, i, a.n, aly);
      Pack<T> f = ld_pack_user(a.F, i, a.n, alf);
      Pack<T> u[PHIV_TAYLOR_PMAX];
      if (pa.mask) phiv_load<T>(pa, i, u);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        T v, y;
        taylor_product(acc.v[k], a.mu, xi.v[k], a.c, v, y);
        if (pa.mask) phiv_add<T>(pa, u, k, y);
        acc.v[k] = y;
        f.v[k] = add_as_written(f.v[k], y);
        if (i + k < a.n) {
          note_abs(abs_T(y), mv, nan, 1u);
          note_abs(abs_T(f.v[k]), mf, nan, 2u);
        }
      }
      st_pack_user(a.y, i, a.n, aly, acc);
      st_pack_user(a.F, i, a.n, alf, f);
    }
  }
  if (taylor_arrive(a.st, mv, mf, nan) && threadIdx.x == 0) taylor_term_test(a.st, a.tol, a.j, a.m, pa.tail);
}

// |z| CORRECTLY ROUNDED, so that U, Wmax and with them nu are the same bits on every platform (hypot is good to an ulp, and which
// ulp differs between math libraries): h = sqrt(a^2 + b^2) to an ulp, then one Newton step with the residual a^2 + b^2 - h^2 taken
// exactly (products split by fma, the sum by its rounding error; s - h^2 is a difference of neighbours).  Scaled by a power of two,
// so nothing overflows; a b that underflows is far below half an ulp of a.
__device__ __forceinline__ double phiv_abs(double re, double im) {
#pragma clang fp contract(off)      // every product and sum below is meant as written: a fused one would count its error twice
  if (re != re || im != im) return __longlong_as_double(0x7ff8000000000000ll);
  double a = fmax(fabs(re), fabs(im)), b = fmin(fabs(re), fabs(im));
  if (a == 0.0 || !(a < __longlong_as_double(0x7ff0000000000000ll))) return a;
  int e;
  a = frexp(a, &e);
  b = ldexp(b, -e);
  const double a2 = a * a, ea = fma(a, a, -a2), b2 = b * b, eb = fma(b, b, -b2);
  const double s = a2 + b2, es = b2 - (s - a2);
  double h = sqrt(s);
  const double h2 = h * h, eh = fma(h, h, -h2);
  h += ((s - h2) + ((es + ea) + (eb - eh))) / (2.0 * h);
  return ldexp(h, e);
}
__device__ __forceinline__ double phiv_abs(double v) { return fabs(v); }
__device__ __forceinline__ double phiv_abs(float v) { return (double)fabsf(v); }
__device__ __forceinline__ double phiv_abs(cplx v) { return phiv_abs(v.re, v.im); }
__device__ __forceinline__ double phiv_abs(cplx32 v) { return phiv_abs((double)v.re, (double)v.im); }

// The plan's two launches (k_taylor_shift_norm with the block's part).  kind 0: CSR arrays, 1: the dense column-major block `val`,
// 2: no stored operator (mode 0 only).  B: column-major, columns 1 .. p are read.
//   mode 0   the trace (per-workgroup partials, finished in index order by the last workgroup) -> mu = tr(A) / (n + p);
//            U = max |u_k[i]| and Wmax = max_i sum_k |u_k[i]| -> umax, wmax of the state
//   mode 1   max_i (|a_ii - mu| + sum_{j != i} |a_ij| + nu sum_k |u_k[i]|), nu from wmax -> rowmax
// A NaN among the sums sets bit 2 of nanflags, which stays set for the host.
template <class T>
__global__ __launch_bounds__(BLOCK) void k_phiv_plan(int mode, int kind, int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const T *__restrict__ val, int64_t lda, const T *__restrict__ B, int64_t ldb, int p, double *part,
                                                    TaylorState *st) {
  __shared__ double red_s[BLOCK / 64];
  const cplx mu = make_cplx(mode ? ts_loadf(&st->mu_re) : 0.0, mode ? ts_loadf(&st->mu_im) : 0.0);
  const double nu = mode ? phiv_nu(ts_loadf(&st->wmax)) : 0.0;
  double tr_re = 0.0, tr_im = 0.0, best = 0.0, umax = 0.0;
  unsigned nan = 0u;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * BLOCK) {
    double d_re = 0.0, d_im = 0.0, off = 0.0, bsum = 0.0;
    auto take = [&](T v, bool diag) {
      if (diag) {
        if constexpr (ST<T>::is_complex) { d_re += (double)v.re; d_im += (double)v.im; }
        else d_re += (double)v;
      } else if (mode) {
        off += abs_T(v);
      }
    };
    if (kind == 0) {
      for (int32_t k = rp[r]; k < rp[r + 1]; ++k) take(val[k], ci[k] == (int32_t)r);
    } else if (kind == 1 && mode) {
      for (int64_t j = 0; j < n; ++j) take(val[r + j * lda], j == r);
    } else if (kind == 1) {
      take(val[r + r * lda], true);
    }
    for (int k = 1; k <= p; ++k) {
      const double a = phiv_abs(B[r + (int64_t)k * ldb]);
      if (!mode) note_abs(a, umax, nan, 4u);
      bsum += a;
    }
    tr_re += d_re;
    tr_im += d_im;
    if (mode) note_abs(off + hypot(d_re - mu.re, d_im - mu.im) + nu * bsum, best, nan, 4u);
    else note_abs(bsum, best, nan, 4u);
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
  if (!taylor_arrive(st, umax, best, nan)) return;
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
    ts_storef(&st->mu_re, s_re / (double)(n + p));
    ts_storef(&st->mu_im, s_im / (double)(n + p));
    ts_store(&st->umax, ts_load(&st->maxv));
    ts_store(&st->wmax, ts_load(&st->maxf));
    const unsigned long long nf = ts_load(&st->nanflags);
    taylor_rearm(st);
    ts_store(&st->nanflags, nf & 4ull);
  }
}

}  // namespace dev

namespace {

struct PhivPlan {
  double nu = 1.0, U = 0.0;
};

// The complex products of the host side, spelled out (see taylor_stage_factor, taylor_state.h: written as a * b the host compiler
// fuses one product of each component and picks which one from the code around).  A product that only feeds an fma leaves nothing
// to contract.  phiv_cmul(a, z): what multiplies the tail zeta.  phiv_stage_factor: exp(mu h); its real part fuses the OTHER
// product, as this file's factor always has -- it is not taylor_stage_factor's, and one-column calls do not come here.
inline std::complex<double> phiv_cmul(std::complex<double> a, std::complex<double> z) {
  const double pr = a.imag() * z.imag(), pi = a.real() * z.imag();
  return std::complex<double>(std::fma(a.real(), z.real(), -pr), std::fma(a.imag(), z.real(), pi));
}
inline std::complex<double> phiv_stage_factor(std::complex<double> mu, std::complex<double> h) {
  const double pr = mu.real() * h.real(), pi = mu.real() * h.imag();
  return std::exp(std::complex<double>(std::fma(-mu.imag(), h.imag(), pr), std::fma(mu.imag(), h.real(), pi)));
}

// mu, alpha, nu, U (two launches and one blocking read; a matrix-free operator: one launch) and (m*, s).  Bd: the block in the
// operator's ordering, column-major.  `head`: taylor_head_bytes() of device memory; its state is ready for the first closing launch.
template <class T>
void phiv_plan_T(Ctx *c, Op &op, std::complex<double> t, const T *Bd, int64_t ldb, int p, int precision, int64_t max_matvecs, double opnorm,
                 void *head, TaylorCall &tc, PhivPlan &pp) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  dev::TaylorState *st = reinterpret_cast<dev::TaylorState *>(head);
  double *part = reinterpret_cast<double *>(static_cast<char *>(head) + sizeof(dev::TaylorState));
  HIPCHECK(hipMemsetAsync(st, 0, sizeof(dev::TaylorState), s));
  const bool stored = op.kind != OP_CALLBACK, dense = op.kind == OP_DENSE;
  if (stored && !dense && !(op.rowptr.p && (op.nnz == 0 || (op.col.p && op.val.p))))
    fail(EXPV_MI_ARGUMENT_ERROR, "expv_taylor: sparse operator without its CSR arrays");
  const int g = dev::taylor_grid(n, dev::BLOCK);
  for (int mode = 0; mode < (stored ? 2 : 1); ++mode) {
    ProfScope ps(c, EXPV_MI_K_LINCOMB);
    hipLaunchKernelGGL(dev::k_phiv_plan<T>, dim3(g), dim3(dev::BLOCK), 0, s, mode, stored ? (dense ? 1 : 0) : 2, n,
                       stored && !dense ? op.rowptr.as<int32_t>() : nullptr, stored && !dense ? op.col.as<int32_t>() : nullptr,
                       !stored ? nullptr : dense ? reinterpret_cast<const T *>(op.dense_ptr) : op.val.as<T>(), dense ? op.lda : (int64_t)0, Bd, ldb, p,
                       part, st);
  }
  dev::TaylorState h;
  HIPCHECK(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  ++tc.reads;
  const std::complex<double> mu = stored ? std::complex<double>(f64_of(h.mu_re), f64_of(h.mu_im)) : std::complex<double>(0.0, 0.0);
  const double wmax = f64_of(h.wmax);
  pp.U = f64_of(h.umax);
  pp.nu = phiv_nu(wmax);
  double anorm = stored ? f64_of(h.rowmax) : opnorm + pp.nu * wmax;
  anorm = std::max(anorm, 1.0 + std::abs(mu));      // the rows of J - mu I
  if (h.nanflags & 4ull) {
    anorm = std::numeric_limits<double>::quiet_NaN();
    pp.U = anorm;
  }
  tc.mu_re = mu.real();
  tc.mu_im = mu.imag();
  tc.alpha = std::abs(t) * anorm;
  if (std::abs(t) == 0.0) tc.alpha = 0.0;      // (0 * Inf: t = 0 returns u_0 whatever A and B hold)
  taylor_choose(op, precision, max_matvecs, tc);
}

// every launch of the series behind the plan: F = v = u_0, then s stages of m* terms and a closing launch
template <class T>
void phiv_run_T(Ctx *c, Op &op, std::complex<double> t, const T *Bd, int64_t ldb, int p, const PhivPlan &pp, void *state, void *v0, void *v1,
                void *Fv, TaylorCall &tc) {
  T *V[2] = {reinterpret_cast<T *>(v0), reinterpret_cast<T *>(v1)};
  const std::complex<double> mu(tc.mu_re, tc.mu_im);
  const int m = tc.m;
  const int64_t ns = tc.s;
  const std::complex<double> h = t / (double)ns;
  const TaylorLaunch<T> L(c, op, tc, reinterpret_cast<T *>(Fv), reinterpret_cast<dev::TaylorState *>(state));
  dev::PhivTermArgs<T> pa{};
  dev::TaylorTermArgs<T> &a = pa.t;
  a = L.args();
  pa.B = Bd; pa.ldb = ldb;
  const std::complex<double> eta = phiv_stage_factor(mu, h);

  // the tail at the start of a stage: zeta[i - 1] = tau^(p - i) / (p - i)!, i = 1 .. p
  std::complex<double> zeta[PHIV_TAYLOR_PMAX], next[PHIV_TAYLOR_PMAX];
  auto stage_tail = [&](int64_t stage) {
    const std::complex<double> tau = (double)stage * h;
    if (p > 0) zeta[p - 1] = 1.0;
    for (int i = p - 1; i >= 1; --i) zeta[i - 1] = phiv_cmul(tau, zeta[i]) / (double)(p - i);
  };
  auto tail_norm = [&] {
    double z = 0.0;
    for (int i = 0; i < p; ++i) z = std::max(z, std::abs(zeta[i]));
    return z * pp.U;
  };
  int q = 0;
  stage_tail(0);
  L.close(Bd, V[0], eta, -1, tail_norm());      // (zeta: the tail of the stage that follows)
  for (int64_t stage = 0; stage < ns; ++stage) {
    for (int j = 1; j <= m; ++j) {
      const std::complex<double> cj = h / (double)j;
      pa.mask = 0u;
      for (int k = 1; k <= p; ++k) {      // u_k takes g_j[p + 1 - k] = c_j zeta_{j-1}[p + 1 - k]
        pa.g[k - 1] = taylor_scalar<T>(phiv_cmul(cj, zeta[p - k]));
        if (!(ST<T>::abs2(pa.g[k - 1]) == 0)) pa.mask |= 1u << (k - 1);
      }
      for (int i = 0; i < p; ++i) next[i] = phiv_cmul(cj, (i + 1 < p ? zeta[i + 1] : std::complex<double>(0.0, 0.0)) - phiv_cmul(mu, zeta[i]));
      for (int i = 0; i < p; ++i) zeta[i] = next[i];
      pa.tail = tail_norm();
      a.x = V[q]; a.y = V[1 - q]; a.j = j;
      a.c = taylor_scalar<T>(cj);
      L.term(pa, a.x, a.y, [](auto fused) { return dev::k_phiv_term<T, decltype(fused)::value>; });
      q ^= 1;
    }
    stage_tail(stage + 1);
    L.close(L.F, V[q], eta, stage, tail_norm());
  }
  HIPCHECK(hipGetLastError());
}

}  // namespace

void phiv_taylor_run(Ctx *c, Op &op, double t_re, double t_im, const void *B, int64_t ldb, int ncols, int b_layout, int b_loc, void *w, int w_loc,
                     int precision, int64_t max_matvecs, double opnorm, int64_t info[8], double dinfo[8]) {
  hipStream_t s = c->stream;
  const int64_t n = op.n;
  const int p = ncols - 1;
  const size_t esz = dtype_size(op.dtype), bytes = (size_t)n * esz;
  const bool colmajor = b_layout == EXPV_MI_BLOCK_COL_MAJOR;
  TaylorCall tc;
  PhivPlan pp;
  DevBuf bhost, bstage, out;
  try {
    taylor_check(op, t_im, precision, opnorm);
    // B where the kernels read it: on the device, column-major, rows in the operator's ordering.  A column-major device block of an
    // operator in its natural ordering is used where it lies; a host block is copied, a row-major one transposed, a reordered
    // operator's permuted, once, into a staging copy whose columns start on 16-byte boundaries.
    const char *Bd = static_cast<const char *>(B);
    int64_t ld = ldb;
    if (b_loc == EXPV_MI_HOST) {
      const int64_t ldc = colmajor ? n : (int64_t)ncols;      // compact, in the caller's layout
      bhost.take_from(c, (size_t)n * (size_t)ncols * esz + 16);
      HIPCHECK(hipMemcpy2DAsync(bhost.p, (size_t)ldc * esz, B, (size_t)ldb * esz, (size_t)ldc * esz, (size_t)(colmajor ? (int64_t)ncols : n),
                                hipMemcpyHostToDevice, s));
      Bd = bhost.as<char>();
      ld = ldc;
    }
    if (!colmajor || op.perm) {
      const int64_t ldx = (int64_t)(up16(bytes) / esz);
      bstage.take_from(c, (size_t)ncols * (size_t)ldx * esz + 16);
      taylor_block_copy(c, op, Bd, colmajor ? 1 : ld, colmajor ? ld : 1, bstage.p, 1, ldx, op.perm ? op.perm->p.as<int32_t>() : nullptr, ncols);
      Bd = bstage.as<char>();
      ld = ldx;
    }
    const size_t vbytes = up16(bytes) + 16, head = taylor_head_bytes();
    tc.work.take_from(c, head + 3 * vbytes);
    char *base = tc.work.as<char>();
    tc.state = base;
    tc.F = base + head + 2 * vbytes;
    if (p == 0) {      // exp(tA) u_0: the loop of expv_taylor.hip itself (mu = tr(A) / n, its alpha, no add)
      taylor_shift_plan(c, op, t_re, t_im, precision, max_matvecs, opnorm, base, tc);
      taylor_run(c, op, t_re, t_im, Bd, base, base + head, base + head + vbytes, tc.F, tc);
    } else {
      dispatch_dtype(op.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const std::complex<double> t(t_re, t_im);
        phiv_plan_T<T>(c, op, t, reinterpret_cast<const T *>(Bd), ld, p, precision, max_matvecs, opnorm, base, tc, pp);
        phiv_run_T<T>(c, op, t, reinterpret_cast<const T *>(Bd), ld, p, pp, base, base + head, base + head + vbytes, tc.F, tc);
      });
    }
    // the result goes to the caller behind the last launch and shares the wait of the state read-back
    const void *src = tc.F;
    if (op.perm) {      // stored as P A P': rows back to their natural places
      void *dst = w;
      if (w_loc == EXPV_MI_HOST) { out.take_from(c, bytes + 16); dst = out.p; }
      dev::gather_rows(s, esz, dst, n, tc.F, n, op.perm->pinv.as<int32_t>(), n, 1);
      src = (w_loc == EXPV_MI_HOST) ? dst : nullptr;
    }
    if (src) HIPCHECK(hipMemcpyAsync(w, src, bytes, w_loc == EXPV_MI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    double d4[4];
    taylor_collect(c, tc, info, d4);
    if (dinfo) {
      for (int k = 0; k < 4; ++k) dinfo[k] = d4[k];
      dinfo[4] = pp.nu;
      dinfo[5] = pp.U;
    }
  } catch (...) {
    (void)hipStreamSynchronize(s);      // (the work vectors go back to the context: nothing may still be writing them)
    throw;
  }
}

}  // namespace expv_mi
