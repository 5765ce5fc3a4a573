// dense_dev.hip -- dense matrices that live on the device: C = alpha A B + beta C on the gfx950 matrix cores (MFMA), a blocked LU
// with partial pivoting built around that product, and exponential!(A) for a device matrix on top of both
// (exp.jl:56-58 -> exponential!(A, ExpMethodHigham2005(false)), exp_noalloc.jl:114-168; test/gpu/gputests.jl:22-39).
//
// The algorithm is host_dense.h's expm_higham2005base without gebal / unbalance: opnorm(A, 1) with fp64 column sums, Pade order by
// the thresholds 0.015 / 0.25 / 0.95 / 2.1, above 2.1 s = max(0, ceil(log2(nA / 5.4))) exact scalings by 1/2 and Pade 13, Horner
// in A^2 with the coefficients converted to the element type, (V - U) X = (V + U) by LU with partial pivoting, s squarings.
// s is NOT capped at 8 as in the reference's generated evaluation graphs (they under-scale for nA >= 1382.4): it is unbounded like
// exp_baseexp.jl and the host routine.
//
// Product kernel: one workgroup of 4 waves (2 x 2) per BM x BN tile of C, K in steps of 16 through LDS.  The real planes of a tile
// are kept in LDS as  As[k][BM + 16]  (rows contiguous, as in the column-major source) and  Bs[col][16 + 2]  (k contiguous, as in
// the source): both fill passes read global memory along its contiguous direction, and both fragment reads are free of bank
// conflicts (the 16 rows of a fragment are consecutive words, its k-quads sit 16 words apart mod 32; a B column step is 18 words).
// Edge tiles are zero-filled in LDS and the stores predicated.  Every element type runs v_mfma_*_16x16x4: A / B fragments are one
// value per lane (lane l: index l & 15, k = l >> 4).  The kernel computes C' = B' A' (first operand: B fragment, second: A
// fragment), so the lane index of the accumulator is a ROW of C and a 16-lane group stores 16 consecutive rows of one column.
// Accumulator register r of lane l is column (l >> 4) * 4 + r of the fragment for f32 and (l >> 4) + 4 r for f64.
// Complex types: the fill pass splits (re, im) into two LDS planes; four real MFMA per k-step into two accumulators
// (re: Ar Br - Ai Bi, im: Ar Bi + Ai Br), the minus sign applied to the Ai fragment after it is read.
#include <chrono>
#include <cmath>
#include <limits>

#include "engine.h"

namespace expv_mi {
namespace {

// Tile choice of the product kernel: the big tile (128 x 128; ComplexF64: 128 x 64) from this many elements of C on, the small one
// (64 x 64) below.  Measured (profiles/expm_device.txt): at 1024^2 outputs the small tile is 1.7 - 3 x faster for every type (the
// big one leaves 3/4 of the CUs idle); at 4096^2 the big tile wins for Float32 (103 vs 88 TFLOP/s) and loses 3 - 9 % for the other
// three types, which therefore stay on the small tile at every size (BigTile<T>::by_size).
constexpr int64_t GEMM_BIG_TILE_MIN_OUTPUTS = (int64_t)4096 * 4096;

constexpr int GEMM_THREADS = 256, GEMM_BK = 16, GEMM_LDB = GEMM_BK + 2, GEMM_APAD = 16;
constexpr int LU_NB = 32;            // panel width of the LU, block size of the triangular solves
constexpr int PANEL_THREADS = 512, EW_THREADS = 256, TRS_THREADS = 64;

template <class R> struct Mfma;
template <> struct Mfma<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  __device__ static inline acc_t run(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  __device__ static inline int reg_index(int lane, int r) { return (lane >> 4) * 4 + r; }
};
template <> struct Mfma<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  __device__ static inline acc_t run(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  __device__ static inline int reg_index(int lane, int r) { return (lane >> 4) + 4 * r; }      // NOT the f32 map
};

__device__ inline float re_of(float a) { return a; }
__device__ inline float im_of(float) { return 0.0f; }
__device__ inline double re_of(double a) { return a; }
__device__ inline double im_of(double) { return 0.0; }
__device__ inline float re_of(cplx32 a) { return a.re; }
__device__ inline float im_of(cplx32 a) { return a.im; }
__device__ inline double re_of(cplx a) { return a.re; }
__device__ inline double im_of(cplx a) { return a.im; }
template <class T, class R> __device__ inline T make_T(R re, R im);
template <> __device__ inline float make_T<float, float>(float re, float) { return re; }
template <> __device__ inline double make_T<double, double>(double re, double) { return re; }
template <> __device__ inline cplx32 make_T<cplx32, float>(float re, float im) { return make_cplx32(re, im); }
template <> __device__ inline cplx make_T<cplx, double>(double re, double im) { return make_cplx(re, im); }

// ---------------------------------------------------------------------------------------------- product
template <class T, int BM, int BN>
__global__ __launch_bounds__(GEMM_THREADS) void gemm_mfma(int64_t m, int64_t n, int64_t k, T alpha, const T *__restrict__ A, int64_t lda,
                                                          const T *__restrict__ B, int64_t ldb, T beta, int beta_zero, T *C, int64_t ldc) {
  using R = typename ST<T>::real_t;
  using MF = Mfma<R>;
  using acc_t = typename MF::acc_t;
  constexpr int NP = ST<T>::nreal;
  constexpr int LDA_S = BM + GEMM_APAD;
  constexpr int FM = BM / 32, FN = BN / 32, WM = BM / 2, WN = BN / 2;
  constexpr int NA = BM * GEMM_BK / GEMM_THREADS, NB = BN * GEMM_BK / GEMM_THREADS;
  static_assert(BM % 32 == 0 && BN % 32 == 0 && NA >= 1 && NB >= 1, "tile shape");
  __shared__ R As[NP][GEMM_BK][LDA_S];
  __shared__ R Bs[NP][BN][GEMM_LDB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, lq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * BM, col0 = (int64_t)blockIdx.y * BN;

  acc_t acc[NP][FM][FN];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[p][i][j] = acc_t{0, 0, 0, 0};

  T ra[NA], rb[NB];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + i * GEMM_THREADS;
      const int64_t r = row0 + (e % BM), kk = k0 + (e / BM);
      ra[i] = (r < m && kk < k) ? A[r + kk * lda] : ST<T>::zero();
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + i * GEMM_THREADS;
      const int64_t kk = k0 + (e % GEMM_BK), c = col0 + (e / GEMM_BK);
      rb[i] = (c < n && kk < k) ? B[kk + c * ldb] : ST<T>::zero();
    }
  };
  fetch(0);
  for (int64_t k0 = 0; k0 < k; k0 += GEMM_BK) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + i * GEMM_THREADS;
      As[0][e / BM][e % BM] = re_of(ra[i]);
      if constexpr (NP == 2) As[1][e / BM][e % BM] = im_of(ra[i]);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int e = tid + i * GEMM_THREADS;
      Bs[0][e / GEMM_BK][e % GEMM_BK] = re_of(rb[i]);
      if constexpr (NP == 2) Bs[1][e / GEMM_BK][e % GEMM_BK] = im_of(rb[i]);
    }
    __syncthreads();
    if (k0 + GEMM_BK < k) fetch(k0 + GEMM_BK);      // the next tile's loads fly under this tile's MFMA
#pragma unroll
    for (int k4 = 0; k4 < GEMM_BK / 4; ++k4) {
      const int kk = k4 * 4 + lq;
      R a[NP][FM], b[NP][FN];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < FM; ++i) a[p][i] = As[p][kk][wr * WM + i * 16 + l15];
#pragma unroll
        for (int j = 0; j < FN; ++j) b[p][j] = Bs[p][wc * WN + j * 16 + l15][kk];
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          acc[0][i][j] = MF::run(b[0][j], a[0][i], acc[0][i][j]);
          if constexpr (NP == 2) {
            acc[0][i][j] = MF::run(b[1][j], -a[1][i], acc[0][i][j]);
            acc[1][i][j] = MF::run(b[1][j], a[0][i], acc[1][i][j]);
            acc[1][i][j] = MF::run(b[0][j], a[1][i], acc[1][i][j]);
          }
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + wr * WM + i * 16 + l15;
        const int64_t col = col0 + wc * WN + j * 16 + MF::reg_index(lane, r);
        if (row < m && col < n) {
          R im = 0;
          if constexpr (NP == 2) im = acc[1][i][j][r];
          T v = ST<T>::mul(alpha, make_T<T, R>(acc[0][i][j][r], im));
          T *dst = C + row + col * ldc;
          if (!beta_zero) v = ST<T>::add(v, ST<T>::mul(beta, *dst));
          *dst = v;
        }
      }
}

template <class T> struct BigTile { static constexpr int BM = 128, BN = 128; static constexpr bool by_size = false; };
template <> struct BigTile<float> { static constexpr int BM = 128, BN = 128; static constexpr bool by_size = true; };
template <> struct BigTile<cplx> { static constexpr int BM = 128, BN = 64; static constexpr bool by_size = false; };      // two fp64 accumulators per fragment: half the columns

template <class T, class R>
inline T host_T(R re, R im) {
  if constexpr (ST<T>::is_complex) { T v; v.re = re; v.im = im; return v; }
  else return (T)re;
}

template <class T>
void gemm_dev(Ctx *ctx, int64_t m, int64_t n, int64_t k, T alpha, const T *A, int64_t lda, const T *B, int64_t ldb, T beta, bool beta_zero,
              T *C, int64_t ldc) {
  if (m <= 0 || n <= 0) return;
  const bool big = ctx->dense_tile == 2 || (ctx->dense_tile != 1 && BigTile<T>::by_size && m * n >= GEMM_BIG_TILE_MIN_OUTPUTS);
  if (big) {
    constexpr int BM = BigTile<T>::BM, BN = BigTile<T>::BN;
    dim3 grid((unsigned)((m + BM - 1) / BM), (unsigned)((n + BN - 1) / BN));
    gemm_mfma<T, BM, BN><<<grid, GEMM_THREADS, 0, ctx->stream>>>(m, n, k, alpha, A, lda, B, ldb, beta, beta_zero ? 1 : 0, C, ldc);
  } else {
    dim3 grid((unsigned)((m + 63) / 64), (unsigned)((n + 63) / 64));
    gemm_mfma<T, 64, 64><<<grid, GEMM_THREADS, 0, ctx->stream>>>(m, n, k, alpha, A, lda, B, ldb, beta, beta_zero ? 1 : 0, C, ldc);
  }
  HIPCHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------- element-wise kernels
// 16 bytes of the real type: the unit of every element-wise pass where the addresses allow it (the rest: a scalar tail)
template <class R> struct __attribute__((aligned(16))) Pack {
  static constexpr int N = 16 / (int)sizeof(R);
  R v[N];
};
__device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// colsum[j] = sum_i |A[i, j]| in fp64 (one workgroup per column); a non-finite entry makes the sum non-finite
template <class T>
__global__ __launch_bounds__(EW_THREADS) void colsum_abs(const T *__restrict__ A, int64_t lda, int64_t n, double *__restrict__ colsum) {
  using R = typename ST<T>::real_t;
  constexpr int NP = ST<T>::nreal, N = Pack<R>::N;
  const R *col = reinterpret_cast<const R *>(A + (int64_t)blockIdx.x * lda);
  const int64_t len = n * NP;
  auto mag = [](R re, R im) -> double {
    if constexpr (NP == 2) return hypot((double)re, (double)im);
    else return fabs((double)re);
  };
  double s = 0.0;
  int64_t done = 0;
  if (aligned16(col)) {
    const int64_t np = len / N;
    const Pack<R> *pk = reinterpret_cast<const Pack<R> *>(col);
    for (int64_t i = threadIdx.x; i < np; i += EW_THREADS) {
      const Pack<R> p = pk[i];
#pragma unroll
      for (int q = 0; q < N; q += NP) s += mag(p.v[q], NP == 2 ? p.v[q + NP - 1] : R(0));
    }
    done = np * N;
  }
  for (int64_t e = done + (int64_t)threadIdx.x * NP; e < len; e += (int64_t)EW_THREADS * NP) s += mag(col[e], NP == 2 ? col[e + NP - 1] : R(0));
  __shared__ double red[EW_THREADS];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = EW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) colsum[blockIdx.x] = red[0];
}
// out[0] = max_j colsum[j], or NaN when one of them is not finite
__global__ __launch_bounds__(EW_THREADS) void colsum_max(const double *__restrict__ colsum, int64_t n, double *__restrict__ out) {
  double best = 0.0;
  int bad = 0;
  for (int64_t j = threadIdx.x; j < n; j += EW_THREADS) {
    const double v = colsum[j];
    if (!(v < INFINITY)) bad = 1;
    else best = fmax(best, v);
  }
  __shared__ double red[EW_THREADS];
  __shared__ int redbad[EW_THREADS];
  red[threadIdx.x] = best;
  redbad[threadIdx.x] = bad;
  __syncthreads();
  for (int w = EW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
      redbad[threadIdx.x] |= redbad[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = redbad[0] ? (double)NAN : red[0];
}

// dst[:, j] = scale * src[:, j] for n x n blocks with their own leading dimensions (blockIdx.y = column); scale is a power of two
template <class T>
__global__ __launch_bounds__(EW_THREADS) void copy_scale(const T *__restrict__ src, int64_t lds_, T *__restrict__ dst, int64_t ldd, int64_t n,
                                                         typename ST<T>::real_t scale) {
  using R = typename ST<T>::real_t;
  constexpr int N = Pack<R>::N;
  const R *s = reinterpret_cast<const R *>(src + (int64_t)blockIdx.y * lds_);
  R *d = reinterpret_cast<R *>(dst + (int64_t)blockIdx.y * ldd);
  const int64_t len = n * ST<T>::nreal;
  const int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * EW_THREADS;
  int64_t done = 0;
  if (aligned16(s) && aligned16(d)) {
    const int64_t np = len / N;
    for (int64_t i = t; i < np; i += nt) {
      Pack<R> p = reinterpret_cast<const Pack<R> *>(s)[i];
#pragma unroll
      for (int q = 0; q < N; ++q) p.v[q] *= scale;
      reinterpret_cast<Pack<R> *>(d)[i] = p;
    }
    done = np * N;
  }
  for (int64_t e = done + t; e < len; e += nt) d[e] = s[e] * scale;
}

__device__ inline bool is_diag_real_index(int64_t e, int64_t n, int nreal) {      // real word e of a packed n x n matrix: real part of a diagonal entry?
  if (nreal == 2) {
    if (e & 1) return false;
    e >>= 1;
  }
  return e % (n + 1) == 0;
}
// Horner step on packed matrices seen as `total` real words: U += cu P, V += cv P; the first step (init) starts from U = du I,
// V = dv I instead of reading them (pade_evaluate: U(i,i) = C[1], V(i,i) = C[0], then the same update)
template <class R>
__global__ __launch_bounds__(EW_THREADS) void horner_update(R *__restrict__ U, R *__restrict__ V, const R *__restrict__ P, R cu, R cv, R du, R dv,
                                                            int init, int64_t total, int64_t n, int nreal) {
  constexpr int N = Pack<R>::N;
  const int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * EW_THREADS;
  const int64_t np = total / N;
  for (int64_t i = t; i < np; i += nt) {
    const Pack<R> p = reinterpret_cast<const Pack<R> *>(P)[i];
    Pack<R> u, v;
    if (init) {
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const bool dg = is_diag_real_index(i * N + q, n, nreal);
        u.v[q] = dg ? du : R(0);
        v.v[q] = dg ? dv : R(0);
      }
    } else {
      u = reinterpret_cast<const Pack<R> *>(U)[i];
      v = reinterpret_cast<const Pack<R> *>(V)[i];
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
      u.v[q] += cu * p.v[q];
      v.v[q] += cv * p.v[q];
    }
    reinterpret_cast<Pack<R> *>(U)[i] = u;
    reinterpret_cast<Pack<R> *>(V)[i] = v;
  }
  for (int64_t e = np * N + t; e < total; e += nt) {
    const bool dg = init && is_diag_real_index(e, n, nreal);
    const R u0 = init ? (dg ? du : R(0)) : U[e], v0 = init ? (dg ? dv : R(0)) : V[e];
    U[e] = u0 + cu * P[e];
    V[e] = v0 + cv * P[e];
  }
}
// in place: (U, V) -> (X, D) = (V + U, V - U)
template <class R>
__global__ __launch_bounds__(EW_THREADS) void sum_diff(R *__restrict__ U, R *__restrict__ V, int64_t total) {
  constexpr int N = Pack<R>::N;
  const int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * EW_THREADS;
  const int64_t np = total / N;
  for (int64_t i = t; i < np; i += nt) {
    const Pack<R> u = reinterpret_cast<const Pack<R> *>(U)[i], v = reinterpret_cast<const Pack<R> *>(V)[i];
    Pack<R> x, d;
#pragma unroll
    for (int q = 0; q < N; ++q) {
      x.v[q] = v.v[q] + u.v[q];
      d.v[q] = v.v[q] - u.v[q];
    }
    reinterpret_cast<Pack<R> *>(U)[i] = x;
    reinterpret_cast<Pack<R> *>(V)[i] = d;
  }
  for (int64_t e = np * N + t; e < total; e += nt) {
    const R u = U[e], v = V[e];
    U[e] = v + u;
    V[e] = v - u;
  }
}

// ---------------------------------------------------------------------------------------------- the solve
// pivot weight: |x| for the real types, |re| + |im| for the complex ones (LAPACK's cabs1, what izamax compares)
template <class T> __device__ inline double pivot_weight(T a) {
  if constexpr (ST<T>::is_complex) return fabs((double)a.re) + fabs((double)a.im);
  else return fabs((double)a);
}
template <class T> __device__ inline T div_T(T a, T b) {
  if constexpr (ST<T>::is_complex) {      // Smith's form: no overflow of |b|^2
    using R = typename ST<T>::real_t;
    if (fabs((double)b.re) >= fabs((double)b.im)) {
      const R r = b.im / b.re, d = b.re + b.im * r;
      return make_T<T, R>((a.re + a.im * r) / d, (a.im - a.re * r) / d);
    }
    const R r = b.re / b.im, d = b.re * r + b.im;
    return make_T<T, R>((a.re * r + a.im) / d, (a.im * r - a.re) / d);
  } else {
    return a / b;
  }
}

// LU with partial pivoting of the panel D[j0:n, j0:j0+jb] by ONE workgroup (unblocked, right-looking inside the panel).  Row
// exchanges are applied to the panel's own columns here and recorded in ipiv (absolute rows); stat[0] counts them, stat[1] becomes
// 1 + column at the first exactly zero pivot column (that column is left as it is, like getrf does).
// A column step costs two barriers: the pivot candidates of column c + 1 are collected while the rank-1 update of step c writes
// that column (each thread keeps the first maximal weight of its own ascending rows), reduced inside each wave by lane exchanges
// and across the waves through a double-buffered LDS slot that every thread reads for itself; the row exchange and the load of
// the pivot row are one pass.  The first maximal weight wins, as in LAPACK.
template <class T>
__global__ __launch_bounds__(PANEL_THREADS) void lu_panel(T *D, int64_t ld, int64_t n, int64_t j0, int jb, int32_t *__restrict__ ipiv,
                                                          int32_t *__restrict__ stat) {
  constexpr int NW = PANEL_THREADS / 64;
  T *P = D + j0 + j0 * ld;
  const int64_t mrows = n - j0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double wbest[2][NW];
  __shared__ int64_t ibest[2][NW];
  __shared__ T urow[LU_NB];
  auto better = [](double x, int64_t xi, double w, int64_t wi) {      // (a NaN weight is taken once and then sticks)
    return x > w || (x == w && xi < wi) || (x != x && w == w);
  };
  int nswap = 0, first_zero = 0;
  double w = -1.0;
  int64_t wi = mrows;
  for (int64_t i = tid; i < mrows; i += PANEL_THREADS) {
    const double x = pivot_weight(P[i]);
    if (better(x, i, w, wi)) { w = x; wi = i; }
  }
  for (int c = 0; c < jb; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ow = __shfl_xor(w, off);
      const long long oi = __shfl_xor((long long)wi, off);
      if (better(ow, (int64_t)oi, w, wi)) { w = ow; wi = (int64_t)oi; }
    }
    if (lane == 0) { wbest[c & 1][wave] = w; ibest[c & 1][wave] = wi; }
    __syncthreads();      // (also: the update of step c - 1 is complete and visible to the whole workgroup)
    double bw = wbest[c & 1][0];
    int64_t bi = ibest[c & 1][0];
#pragma unroll
    for (int v = 1; v < NW; ++v) {
      const double ow = wbest[c & 1][v];
      const int64_t oi = ibest[c & 1][v];
      if (better(ow, oi, bw, bi)) { bw = ow; bi = oi; }
    }
    const bool zero = (bw == 0.0) || bi >= mrows;
    const int64_t p = zero ? c : bi;
    if (tid == 0) {
      ipiv[j0 + c] = (int32_t)(j0 + p);
      if (p != c) ++nswap;
      if (zero && first_zero == 0) first_zero = (int)(j0 + c + 1);
    }
    if (tid < jb) {      // exchange rows c and p of the panel; the new row c is the pivot row
      T *q = P + (int64_t)tid * ld;
      const T vp = q[p];
      if (p != c) { q[p] = q[c]; q[c] = vp; }
      urow[tid] = vp;
    }
    __syncthreads();
    w = -1.0;
    wi = mrows;
    if (!zero) {
      const T pivot = urow[c];
      for (int64_t i = c + 1 + tid; i < mrows; i += PANEL_THREADS) {
        const T l = div_T(P[i + (int64_t)c * ld], pivot);
        P[i + (int64_t)c * ld] = l;
        for (int cc = c + 1; cc < jb; ++cc) {
          T v = P[i + (int64_t)cc * ld];
          ST<T>::nfma(v, l, urow[cc]);
          P[i + (int64_t)cc * ld] = v;
          if (cc == c + 1) {
            const double x = pivot_weight(v);
            if (better(x, i, w, wi)) { w = x; wi = i; }
          }
        }
      }
    } else if (c + 1 < jb) {      // nothing to eliminate with: the next column's candidates are what is stored
      for (int64_t i = c + 1 + tid; i < mrows; i += PANEL_THREADS) {
        const double x = pivot_weight(P[i + (int64_t)(c + 1) * ld]);
        if (better(x, i, w, wi)) { w = x; wi = i; }
      }
    }
  }
  if (tid == 0) {
    stat[0] = stat[0] + nswap;
    if (first_zero != 0 && stat[1] == 0) stat[1] = first_zero;
  }
}

// the panel's row exchanges on columns [0, ncols) of M (one thread per column, the exchanges in order)
template <class T>
__global__ __launch_bounds__(EW_THREADS) void apply_row_swaps(T *__restrict__ M, int64_t ld, int64_t ncols, const int32_t *__restrict__ ipiv, int64_t j0,
                                                              int jb) {
  const int64_t c = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
  if (c >= ncols) return;
  T *col = M + c * ld;
  for (int q = 0; q < jb; ++q) {
    const int64_t r = j0 + q, p = ipiv[r];
    if (p != r) {
      const T t = col[r];
      col[r] = col[p];
      col[p] = t;
    }
  }
}

// LU_NB values of one column held in registers (every index an unrolled constant).  The complex types keep two real arrays: an array
// of (re, im) structs ends up in scratch.
template <class T, bool CX = ST<T>::is_complex> struct ColRegs;
template <class T> struct ColRegs<T, false> {
  T v[LU_NB];
  __device__ inline T get(int i) const { return v[i]; }
  __device__ inline void set(int i, T x) { v[i] = x; }
};
template <class T> struct ColRegs<T, true> {
  using R = typename ST<T>::real_t;
  R re[LU_NB], im[LU_NB];
  __device__ inline T get(int i) const { return make_T<T, R>(re[i], im[i]); }
  __device__ inline void set(int i, T x) { re[i] = x.re; im[i] = x.im; }
};

// B[0:jb, c] <- inv(Tri) B[0:jb, c] for every column c < ncols (one thread per column, the block's rows in registers): Tri is the
// jb x jb block at `tri`, UNIT lower triangular (UPPER = false: forward substitution, the diagonal is not read) or upper triangular
// (UPPER = true: back substitution).  Blocks narrower than LU_NB are padded with the identity.
template <class T, bool UPPER>
__global__ __launch_bounds__(TRS_THREADS) void tri_solve_block(const T *__restrict__ tri, int64_t ldt, int jb, T *__restrict__ B, int64_t ldb, int64_t ncols) {
  __shared__ T Ts[LU_NB][LU_NB + 1];
  for (int e = threadIdx.x; e < LU_NB * LU_NB; e += TRS_THREADS) {
    const int i = e % LU_NB, j = e / LU_NB;
    T v = ST<T>::zero();
    if (i < jb && j < jb) v = tri[i + (int64_t)j * ldt];
    else if (i == j) v = ST<T>::from_real(1.0);
    Ts[i][j] = v;
  }
  __syncthreads();
  const int64_t c = (int64_t)blockIdx.x * TRS_THREADS + threadIdx.x;
  if (c >= ncols) return;
  T *col = B + c * ldb;
  ColRegs<T> b;
#pragma unroll
  for (int i = 0; i < LU_NB; ++i) b.set(i, (i < jb) ? col[i] : ST<T>::zero());
  // the step index r stays a run-time value (one copy of the loop body) while the registers are only ever indexed by unrolled
  // constants: the value the NEXT step eliminates with is caught as it is produced
  if constexpr (!UPPER) {
    T br = b.get(0);
#pragma unroll 1
    for (int r = 0; r < jb; ++r) {
      T nxt = br;
#pragma unroll
      for (int i = 1; i < LU_NB; ++i)
        if (i > r) {
          T bi = b.get(i);
          ST<T>::nfma(bi, Ts[i][r], br);
          b.set(i, bi);
          if (i == r + 1) nxt = bi;
        }
      br = nxt;
    }
  } else {
    T br = b.get(LU_NB - 1);      // (rows >= jb: zero right-hand side, unit diagonal -- they pass through)
#pragma unroll 1
    for (int r = LU_NB - 1; r >= 0; --r) {
      br = div_T(br, Ts[r][r]);
      T nxt = br;
#pragma unroll
      for (int i = 0; i < LU_NB; ++i) {
        if (i == r) {
          b.set(i, br);
        } else if (i < r) {
          T bi = b.get(i);
          ST<T>::nfma(bi, Ts[i][r], br);
          b.set(i, bi);
          if (i == r - 1) nxt = bi;
        }
      }
      br = nxt;
    }
  }
#pragma unroll
  for (int i = 0; i < LU_NB; ++i)
    if (i < jb) col[i] = b.get(i);
}

// D X = X for packed n x n D and X (both overwritten): right-looking blocked LU with partial pivoting.  Per panel: factor it (one
// workgroup), exchange the rows of the columns to its right and of X, block row of U and of L^-1 P X by a unit-lower solve, trailing
// update of D and of the rows of X below through the product kernel (alpha = -1, beta = 1) -- the forward substitution of the n
// right-hand sides rides along with the factorisation.  Then back substitution, blocked the same way.
template <class T>
void lu_solve_dev(Ctx *ctx, int64_t n, T *D, T *X, int32_t *ipiv, int32_t *stat) {
  hipStream_t s = ctx->stream;
  const T one = host_T<T, double>(1.0, 0.0), minus_one = host_T<T, double>(-1.0, 0.0);
  for (int64_t j0 = 0; j0 < n; j0 += LU_NB) {
    const int jb = (int)std::min<int64_t>(LU_NB, n - j0);
    const int64_t right = n - j0 - jb;      // columns right of / rows below the panel
    lu_panel<T><<<1, PANEL_THREADS, 0, s>>>(D, n, n, j0, jb, ipiv, stat);
    if (right > 0) apply_row_swaps<T><<<(unsigned)((right + EW_THREADS - 1) / EW_THREADS), EW_THREADS, 0, s>>>(D + (j0 + jb) * n, n, right, ipiv, j0, jb);
    apply_row_swaps<T><<<(unsigned)((n + EW_THREADS - 1) / EW_THREADS), EW_THREADS, 0, s>>>(X, n, n, ipiv, j0, jb);
    const T *L11 = D + j0 + j0 * n;
    if (right > 0)
      tri_solve_block<T, false><<<(unsigned)((right + TRS_THREADS - 1) / TRS_THREADS), TRS_THREADS, 0, s>>>(L11, n, jb, D + j0 + (j0 + jb) * n, n, right);
    tri_solve_block<T, false><<<(unsigned)((n + TRS_THREADS - 1) / TRS_THREADS), TRS_THREADS, 0, s>>>(L11, n, jb, X + j0, n, n);
    HIPCHECK(hipGetLastError());
    if (right > 0) {
      const T *L21 = D + (j0 + jb) + j0 * n;
      gemm_dev<T>(ctx, right, right, jb, minus_one, L21, n, D + j0 + (j0 + jb) * n, n, one, false, D + (j0 + jb) + (j0 + jb) * n, n);
      gemm_dev<T>(ctx, right, n, jb, minus_one, L21, n, X + j0, n, one, false, X + (j0 + jb), n);
    }
  }
  for (int64_t j0 = ((n - 1) / LU_NB) * LU_NB; j0 >= 0; j0 -= LU_NB) {
    const int jb = (int)std::min<int64_t>(LU_NB, n - j0);
    tri_solve_block<T, true><<<(unsigned)((n + TRS_THREADS - 1) / TRS_THREADS), TRS_THREADS, 0, s>>>(D + j0 + j0 * n, n, jb, X + j0, n, n);
    HIPCHECK(hipGetLastError());
    if (j0 > 0) gemm_dev<T>(ctx, j0, n, jb, minus_one, D + j0 * n, n, X + j0, n, one, false, X, n);
  }
}

// ---------------------------------------------------------------------------------------------- exponential!(A)
// six n x n matrices + pivots + column sums + status words, kept in the context and grown on demand: a loop of calls allocates nothing
struct DenseWs {
  DevBuf W[6], colsum, ipiv, stat;
  DevBuf phiS, phiT;        // phi!(out, A, k): the slabs [Phi_0 ... Phi_k] and Phi_0 [Phi_0 ... Phi_k]
  DevBuf bal;               // balancing: positions, counts, factors and the BalMeta words (carved by bal_carve)
  void *pin = nullptr;      // pinned host mirror of `stat`
  void *pinbal = nullptr;   // pinned host mirror of the BalMeta words
  void *pinscale = nullptr; // pinned host mirror of rec[] and d[] (expv_mi_gebal's scale vector), grown on demand
  size_t pinscale_bytes = 0;
  ~DenseWs() {
    if (pin) (void)hipHostFree(pin);
    if (pinbal) (void)hipHostFree(pinbal);
    if (pinscale) (void)hipHostFree(pinscale);
  }
};
struct StatWords {      // device `stat` buffer / its host mirror
  double norm1;
  int32_t lu[2];       // row exchanges, 1 + first zero pivot column (0: none)
};

DenseWs *dense_ws(Ctx *ctx) {
  DenseWs *ws = reinterpret_cast<DenseWs *>(ctx->ws_dense);
  if (!ws) {
    ws = new DenseWs();
    ctx->ws_dense = ws;
    ctx->ws_dense_free = [](void *q) { delete reinterpret_cast<DenseWs *>(q); };
  }
  return ws;
}

// ---------------------------------------------------------------------------------------------- balancing: xGEBAL job 'B' on the device
// The decisions and their order are host_dense.h's gebal (2-norm variant, radix 2, factor 0.95), made by ONE workgroup; the n^2 work
// around them is parallel.
//   isolation  every exchange of the host routine is a symmetric permutation (the parts of the rows and columns it skips hold zeros),
//              so the matrix is never moved during the search: the off-diagonal nonzeros of every row and column are counted once
//              (-0.0 is zero), bal_peel walks the host's scan order on these counts and a position map pos[] (position -> original
//              index) -- rows i = l .. 1 exchanged with l, then columns j = k .. l exchanged with k -- and lowers the counts by one
//              column of A (or of its transpose) per isolated index.  P is applied once, by a gather (perm_scale).
//   scaling    sequential in i as in LAPACK (each step sees the factors of the steps before it).  The matrix is not rewritten: a step
//              reads column i of P'AP and of its transpose, scales every element by d_i / d_q (or d_q / d_i) on the fly -- exact,
//              the factors are powers of two, so this is bit for bit the eagerly scaled element -- and sums the squares in fp64 for
//              every element type, each thread over its own ascending rows, then lanes, then waves, always in the same order.
//              The guards sfmin1/2, sfmax1/2 are those of the ELEMENT type's real type.
//   loops      the peel runs at most n + 1 passes per phase, the sweeps at most BAL_MAX_SWEEPS (BalMeta.noconv still set then: the
//              driver answers with a status), the two doubling loops of a step are bounded by their own guards.
constexpr int BAL_THREADS = 512;
constexpr int BAL_MAX_SWEEPS = 128;

struct BalMeta {      // device words of one balancing / their pinned host mirror
  int32_t ilo, ihi;   // 1-based, as LAPACK returns them
  int32_t sweeps;     // sweeps of the scaling loop so far (the last one changes nothing)
  int32_t noconv;     // the last sweep changed a factor
  int32_t swaps;      // exchanges of two DIFFERENT positions
  int32_t early;      // the l == 1 return of the row search (no column search, no scaling)
};

template <class T> __device__ inline bool nonzero_T(T a) { return re_of(a) != 0 || im_of(a) != 0; }

// At = A' (plain transpose, no conjugation): packed n x n, through a 32 x 33 LDS tile so that both sides move along their columns
template <class T>
__global__ __launch_bounds__(EW_THREADS) void transpose_to(const T *__restrict__ A, int64_t lda, int64_t n, T *__restrict__ At) {
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
  for (int j = ty; j < 32; j += EW_THREADS / 32)
    if (r0 + tx < n && c0 + j < n) tile[j][tx] = A[(r0 + tx) + (c0 + j) * lda];
  __syncthreads();
  for (int j = ty; j < 32; j += EW_THREADS / 32)
    if (c0 + tx < n && r0 + j < n) At[(c0 + tx) + (r0 + j) * n] = tile[tx][j];
}

// cnt[j] = number of nonzero entries of column j off the diagonal (one workgroup per column)
template <class T>
__global__ __launch_bounds__(EW_THREADS) void offdiag_count(const T *__restrict__ A, int64_t lda, int64_t n, int32_t *__restrict__ cnt) {
  const int64_t j = blockIdx.x;
  const T *col = A + j * lda;
  int c = 0;
  for (int64_t i = threadIdx.x; i < n; i += EW_THREADS)
    if (i != j && nonzero_T(col[i])) ++c;
  __shared__ int red[EW_THREADS];
  red[threadIdx.x] = c;
  __syncthreads();
  for (int w = EW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[j] = red[0];
}

// The permutation phase (one workgroup).  rowcnt / colcnt: offdiag_count of A' and of A, by ORIGINAL index; they are lowered as
// indices leave the active block.  Out: pos[], rec[] (LAPACK's record: rec[m] = 1 + the position exchanged with position m), d[] = dinv[] = 1,
// and the meta words.  Positions are 0-based here, ilo / ihi 1-based.
template <class T>
__global__ __launch_bounds__(BAL_THREADS) void bal_peel(const T *__restrict__ A, int64_t lda, const T *__restrict__ At, int n, int32_t *rowcnt,
                                                        int32_t *colcnt, int32_t *pos, double *rec, double *d, double *dinv, BalMeta *meta) {
  __shared__ int found;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += BAL_THREADS) {
    pos[i] = i;
    rec[i] = 1.0;
    d[i] = 1.0;
    dinv[i] = 1.0;
  }
  __syncthreads();
  int k = 1, l = n, swaps = 0;
  bool early = false;
  for (int pass = 0; pass <= n; ++pass) {      // rows that isolate an eigenvalue go to the bottom
    bool any = false;
    int cur = l - 1;
    while (cur >= 0) {
      int hit = -1;      // the largest position <= cur whose row has no off-diagonal nonzero in the columns 0 .. l-1
      while (cur >= 0) {
        if (tid == 0) found = -1;
        __syncthreads();
        const int p = cur - tid;
        if (p >= 0 && rowcnt[pos[p]] == 0) atomicMax(&found, p);
        __syncthreads();
        const int f = found;
        __syncthreads();
        if (f >= 0) { hit = f; break; }
        cur -= BAL_THREADS;
      }
      if (hit < 0) break;
      const int o = pos[hit], ol = pos[l - 1];
      __syncthreads();
      if (tid == 0) {
        pos[hit] = ol;
        pos[l - 1] = o;
        rec[l - 1] = (double)(hit + 1);
      }
      if (hit != l - 1) ++swaps;
      any = true;
      if (l == 1) { early = true; break; }
      const T *col = A + (int64_t)o * lda;      // column o leaves the active block: one nonzero fewer in the rows that had one there
      for (int i = tid; i < n; i += BAL_THREADS)
        if (i != o && nonzero_T(col[i])) rowcnt[i] -= 1;
      --l;
      cur = hit - 1;
      __syncthreads();
    }
    if (early || !any) break;
  }
  if (!early) {
    for (int pass = 0; pass <= n; ++pass) {      // columns that isolate an eigenvalue go to the left
      bool any = false;
      int cur = k - 1;
      while (cur <= l - 1) {
        int hit = -1;      // the smallest position >= cur whose column has no off-diagonal nonzero in the rows k-1 .. l-1
        while (cur <= l - 1) {
          if (tid == 0) found = 0x7fffffff;
          __syncthreads();
          const int p = cur + tid;
          if (p <= l - 1 && colcnt[pos[p]] == 0) atomicMin(&found, p);
          __syncthreads();
          const int f = found;
          __syncthreads();
          if (f != 0x7fffffff) { hit = f; break; }
          cur += BAL_THREADS;
        }
        if (hit < 0) break;
        const int o = pos[hit], ok = pos[k - 1];
        __syncthreads();
        if (tid == 0) {
          pos[hit] = ok;
          pos[k - 1] = o;
          rec[k - 1] = (double)(hit + 1);
        }
        if (hit != k - 1) ++swaps;
        any = true;
        const T *row = At + (int64_t)o * n;      // row o leaves the active block
        for (int i = tid; i < n; i += BAL_THREADS)
          if (i != o && nonzero_T(row[i])) colcnt[i] -= 1;
        ++k;
        cur = hit + 1;
        __syncthreads();
      }
      if (!any) break;
    }
  }
  if (tid == 0) {
    meta->ilo = early ? 1 : k;
    meta->ihi = early ? 1 : l;
    meta->sweeps = 0;
    meta->noconv = early ? 0 : 1;
    meta->swaps = swaps;
    meta->early = early ? 1 : 0;
  }
}

// wave-wide sum / first maximum by lane exchanges: every lane ends with the same value
__device__ inline double bal_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// (CX: the winning element travels along -- its modulus is needed afterwards; for the real types the weight IS the modulus)
template <bool CX>
__device__ inline void bal_wave_first_max(double &w, int &wi, double &re, double &im) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ow = __shfl_xor(w, off);
    const int oi = __shfl_xor(wi, off);
    double ore = 0.0, oim = 0.0;
    if constexpr (CX) { ore = __shfl_xor(re, off); oim = __shfl_xor(im, off); }
    if (ow > w || (ow == w && oi < wi)) { w = ow; wi = oi; re = ore; im = oim; }
  }
}
// workgroup-wide sum / maximum through buf[BAL_THREADS / 64] (two barriers; every thread returns the same value)
__device__ inline double bal_block_sum(double v, double *buf) {
  v = bal_wave_sum(v);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < BAL_THREADS / 64; ++w) s += buf[w];
  __syncthreads();
  return s;
}
__device__ inline double bal_block_max(double v, double *buf) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = buf[0];
#pragma unroll
  for (int w = 1; w < BAL_THREADS / 64; ++w) s = fmax(s, buf[w]);
  __syncthreads();
  return s;
}
// 2-norm of vec[lo .. hi] with every element times num / d[q] (INV = false) or d[q] / num (INV = true), in the scaled form: only
// where the plain sum of squares leaves (1e-280, 1e280) -- nrm2_strided of the host routine.  dinv[q] = 1 / d[q], inum = 1 / num.
template <class T, bool INV>
__device__ inline double bal_nrm2_scaled(const T *__restrict__ vec, int lo, int hi, const double *d, const double *dinv, double num, double inum,
                                         double *buf) {
  double amax = 0.0;
  for (int q = lo + (int)threadIdx.x; q <= hi; q += BAL_THREADS) {
    const double ratio = INV ? d[q] * inum : num * dinv[q];
    amax = fmax(amax, fmax(fabs((double)re_of(vec[q]) * ratio), fabs((double)im_of(vec[q]) * ratio)));
  }
  amax = bal_block_max(amax, buf);
  if (!(amax > 0.0)) return 0.0;
  double ssq = 0.0;
  for (int q = lo + (int)threadIdx.x; q <= hi; q += BAL_THREADS) {
    const double ratio = INV ? d[q] * inum : num * dinv[q];
    const double re = (double)re_of(vec[q]) * ratio / amax, im = (double)im_of(vec[q]) * ratio / amax;
    ssq += re * re + im * im;
  }
  return amax * sqrt(bal_block_sum(ssq, buf));
}

// The sweeps of the scaling loop (at most BAL_MAX_SWEEPS) over the positions ilo .. ihi (one workgroup).  Ap = P'AP and Apt = its transpose, both
// packed; d[] holds the factors (1 outside ilo .. ihi), dinv[] their reciprocals: the only things written, with the sweep count and
// `noconv`.  d_i / d_q is formed as d_i * (1 / d_q): both are powers of two, so the product is the quotient bit for bit.
template <class T>
__global__ __launch_bounds__(BAL_THREADS) void bal_sweeps(const T *__restrict__ Ap, const T *__restrict__ Apt, int n, double *d, double *dinv, BalMeta *meta,
                                                          double sfmin1, double sfmax1, double sfmin2, double sfmax2) {
  constexpr int NW = BAL_THREADS / 64;
  constexpr bool CX = ST<T>::is_complex;
  __shared__ double s_ssc[NW], s_ssr[NW], s_bc[NW], s_br[NW], s_buf[NW], s_el[4][NW];
  __shared__ int s_ic[NW], s_ir[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = meta->ilo - 1, l0 = meta->ihi - 1;      // first and last active position
  int sweeps = meta->sweeps, noconv = meta->noconv;
  __syncthreads();
  while (noconv && sweeps < BAL_MAX_SWEEPS) {
    noconv = 0;
    for (int i = k0; i <= l0; ++i) {
      const double di = d[i], dii = dinv[i];
      const T *col = Ap + (int64_t)i * n, *row = Apt + (int64_t)i * n;
      double ssc = 0.0, ssr = 0.0, bc = -1.0, br = -1.0, cre = 0.0, cim = 0.0, rre = 0.0, rim = 0.0;
      int ic = 0x7fffffff, ir = 0x7fffffff;
      for (int q = tid; q <= l0; q += BAL_THREADS) {      // column i: rows 0 .. ihi-1 for the largest entry, ilo-1 .. ihi-1 for the norm
        const double ratio = di * dinv[q];
        const double re = (double)re_of(col[q]) * ratio, im = (double)im_of(col[q]) * ratio;
        const double w = fabs(re) + fabs(im);
        if (w > bc) { bc = w; ic = q; cre = re; cim = im; }
        if (q >= k0) ssc += re * re + im * im;
      }
      for (int q = k0 + tid; q < n; q += BAL_THREADS) {   // row i: columns ilo-1 .. n-1 for the largest entry, ilo-1 .. ihi-1 for the norm
        const double ratio = d[q] * dii;
        const double re = (double)re_of(row[q]) * ratio, im = (double)im_of(row[q]) * ratio;
        const double w = fabs(re) + fabs(im);
        if (w > br) { br = w; ir = q; rre = re; rim = im; }
        if (q <= l0) ssr += re * re + im * im;
      }
      ssc = bal_wave_sum(ssc);
      ssr = bal_wave_sum(ssr);
      bal_wave_first_max<CX>(bc, ic, cre, cim);
      bal_wave_first_max<CX>(br, ir, rre, rim);
      if (lane == 0) {
        s_ssc[wave] = ssc; s_ssr[wave] = ssr;
        s_bc[wave] = bc; s_ic[wave] = ic;
        s_br[wave] = br; s_ir[wave] = ir;
        if constexpr (CX) { s_el[0][wave] = cre; s_el[1][wave] = cim; s_el[2][wave] = rre; s_el[3][wave] = rim; }
      }
      __syncthreads();
      ssc = s_ssc[0]; ssr = s_ssr[0]; bc = s_bc[0]; ic = s_ic[0]; br = s_br[0]; ir = s_ir[0];
      int wc = 0, wr = 0;      // the waves that hold the two first maxima
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        ssc += s_ssc[w];
        ssr += s_ssr[w];
        if (s_bc[w] > bc || (s_bc[w] == bc && s_ic[w] < ic)) { bc = s_bc[w]; ic = s_ic[w]; wc = w; }
        if (s_br[w] > br || (s_br[w] == br && s_ir[w] < ir)) { br = s_br[w]; ir = s_ir[w]; wr = w; }
      }
      double c = (ssc > 1e-280 && ssc < 1e280) ? sqrt(ssc) : bal_nrm2_scaled<T, false>(col, k0, l0, d, dinv, di, dii, s_buf);
      double r = (ssr > 1e-280 && ssr < 1e280) ? sqrt(ssr) : bal_nrm2_scaled<T, true>(row, k0, l0, d, dinv, di, dii, s_buf);
      double f = 1.0;
      bool change = false;
      if (c != 0.0 && r != 0.0) {
        double ca = bc, ra = br;      // the modulus of the entry with the largest |re| + |im| (the first one)
        if constexpr (CX) {
          ca = hypot(s_el[0][wc], s_el[1][wc]);
          ra = hypot(s_el[2][wr], s_el[3][wr]);
        }
        double g = r / 2.0;
        const double s = c + r;
        while (c < g && fmax(f, fmax(c, ca)) < sfmax2 && fmin(r, fmin(g, ra)) > sfmin2) {
          f *= 2.0; c *= 2.0; ca *= 2.0; r /= 2.0; g /= 2.0; ra /= 2.0;
        }
        g = c / 2.0;
        while (g >= r && fmax(r, ra) < sfmax2 && fmin(fmin(f, c), fmin(g, ca)) > sfmin2) {
          f /= 2.0; c /= 2.0; g /= 2.0; ca /= 2.0; r *= 2.0; ra *= 2.0;
        }
        change = !((c + r) >= 0.95 * s) && !(f < 1.0 && di < 1.0 && f * di <= sfmin1) && !(f > 1.0 && di > 1.0 && di >= sfmax1 / f);
      }
      if (change) {
        noconv = 1;
        if (tid == 0) {
          d[i] = di * f;
          dinv[i] = 1.0 / (di * f);
        }
      }
      __syncthreads();      // d[i] is visible to the next step, the LDS slots are free again
    }
    ++sweeps;
  }
  if (tid == 0) {
    meta->sweeps = sweeps;
    meta->noconv = noconv;
  }
}

// by position q and by original index o = pos[q]: the inverse map and the four factor vectors of the two element-wise passes
__global__ __launch_bounds__(EW_THREADS) void bal_factors(const int32_t *__restrict__ pos, const double *__restrict__ d, int64_t n, int32_t *__restrict__ inv,
                                                          double *__restrict__ rf, double *__restrict__ cf, double *__restrict__ urf,
                                                          double *__restrict__ ucf) {
  const int64_t q = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
  if (q >= n) return;
  const int32_t o = pos[q];
  const double dq = d[q];
  inv[o] = (int32_t)q;
  rf[q] = 1.0 / dq;      // A_bal[i, j] = (P'AP)[i, j] d_j / d_i
  cf[q] = dq;
  urf[o] = dq;           // exp(A)[i, j] = X[inv i, inv j] d_(inv i) / d_(inv j)
  ucf[o] = 1.0 / dq;
}

template <class R> __device__ inline R scale_pow2(R x, double fac) { return (R)((double)x * fac); }

// dst[i, j] = src[map[i], map[j]] rf[i] cf[j]  (blockIdx.y = column j).  map == nullptr: the identity, and then 16-byte packs where
// both columns are aligned; rf == nullptr: no factors (a pure gather).  rf[i] cf[j] is one power of two in fp64 and the product is
// rounded to the element type once, so the result is the exactly scaled element.  dst == src is allowed when map == nullptr.
// (For the fp64 element types rf[i] cf[j] itself can leave the double range -- factors 2^600 apart and more -- where the host's
// step-by-step scaling of a small enough entry would not; the guards keep each factor inside (sfmin1, sfmax1), not their quotient.)
template <class T>
__global__ __launch_bounds__(EW_THREADS) void perm_scale(const T *src, int64_t lds_, T *dst, int64_t ldd, int64_t n, const int32_t *__restrict__ map,
                                                         const double *__restrict__ rf, const double *__restrict__ cf) {
  using R = typename ST<T>::real_t;
  constexpr int NP = ST<T>::nreal, N = Pack<R>::N;
  const int64_t j = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * EW_THREADS;
  const double cj = rf ? cf[j] : 1.0;
  R *d = reinterpret_cast<R *>(dst + j * ldd);
  if (map) {
    const R *s = reinterpret_cast<const R *>(src + (int64_t)map[j] * lds_);
    for (int64_t i = t; i < n; i += nt) {
      const int64_t si = map[i];
      const double fac = rf ? rf[i] * cj : 1.0;
#pragma unroll
      for (int p = 0; p < NP; ++p) d[i * NP + p] = rf ? scale_pow2<R>(s[si * NP + p], fac) : s[si * NP + p];
    }
    return;
  }
  const R *s = reinterpret_cast<const R *>(src + j * lds_);
  const int64_t len = n * NP;
  int64_t done = 0;
  if (aligned16(s) && aligned16(d)) {
    const int64_t np = len / N;
    for (int64_t i = t; i < np; i += nt) {
      Pack<R> p = reinterpret_cast<const Pack<R> *>(s)[i];
      if (rf) {
#pragma unroll
        for (int q = 0; q < N; ++q) p.v[q] = scale_pow2<R>(p.v[q], rf[(i * N + q) / NP] * cj);
      }
      reinterpret_cast<Pack<R> *>(d)[i] = p;
    }
    done = np * N;
  }
  for (int64_t e = done + t; e < len; e += nt) d[e] = rf ? scale_pow2<R>(s[e], rf[e / NP] * cj) : s[e];
}

struct BalBufs {      // the carved `bal` buffer of the workspace
  int32_t *pos, *inv, *rowcnt, *colcnt;
  double *rec, *d, *dinv, *rf, *cf, *urf, *ucf;
  BalMeta *meta;
};
BalBufs bal_carve(DenseWs *ws, int64_t n) {
  const size_t ni = (((size_t)n * sizeof(int32_t) + 255) / 256) * 256, nd = (((size_t)n * sizeof(double) + 255) / 256) * 256;
  const size_t bytes = 4 * ni + 7 * nd + 256;
  if (ws->bal.bytes < bytes) ws->bal.alloc(bytes);
  if (!ws->pinbal) HIPCHECK(hipHostMalloc(&ws->pinbal, sizeof(BalMeta), hipHostMallocDefault));
  char *p = ws->bal.as<char>();
  BalBufs b;
  b.pos = reinterpret_cast<int32_t *>(p);
  b.inv = reinterpret_cast<int32_t *>(p + ni);
  b.rowcnt = reinterpret_cast<int32_t *>(p + 2 * ni);
  b.colcnt = reinterpret_cast<int32_t *>(p + 3 * ni);
  p += 4 * ni;
  b.rec = reinterpret_cast<double *>(p);
  b.d = reinterpret_cast<double *>(p + nd);
  b.rf = reinterpret_cast<double *>(p + 2 * nd);
  b.cf = reinterpret_cast<double *>(p + 3 * nd);
  b.urf = reinterpret_cast<double *>(p + 4 * nd);
  b.ucf = reinterpret_cast<double *>(p + 5 * nd);
  b.dinv = reinterpret_cast<double *>(p + 6 * nd);
  b.meta = reinterpret_cast<BalMeta *>(p + 7 * nd);
  return b;
}

template <class T>
dim3 column_grid(int64_t n) {
  using R = typename ST<T>::real_t;
  return dim3((unsigned)std::min<int64_t>((n * ST<T>::nreal / Pack<R>::N + EW_THREADS) / EW_THREADS, 64), (unsigned)n);
}

// Balances A (device, leading dimension lda; only read): afterwards Ap holds P'AP (packed, NOT yet scaled), the factor vectors of
// `b` are complete and the meta words are on their way to the pinned mirror -- the caller synchronises the stream before it reads
// them.  At and Apt are scratch (packed n x n).  The sweeps loop inside ONE launch, capped at BAL_MAX_SWEEPS: one launch per sweep with
// `noconv` read back in between was measured too and was slower or equal (profiles/expm_balance_sweep_forms.txt), so it is gone.
template <class T>
void balance_dev(Ctx *ctx, DenseWs *ws, const BalBufs &b, int64_t n, const T *A, int64_t lda, T *At, T *Ap, T *Apt) {
  using R = typename ST<T>::real_t;
  hipStream_t s = ctx->stream;
  BalMeta *hmeta = reinterpret_cast<BalMeta *>(ws->pinbal);
  const dim3 tgrid((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), cgrid = column_grid<T>(n);
  transpose_to<T><<<tgrid, EW_THREADS, 0, s>>>(A, lda, n, At);
  offdiag_count<T><<<(unsigned)n, EW_THREADS, 0, s>>>(A, lda, n, b.colcnt);
  offdiag_count<T><<<(unsigned)n, EW_THREADS, 0, s>>>(At, n, n, b.rowcnt);
  bal_peel<T><<<1, BAL_THREADS, 0, s>>>(A, lda, At, (int)n, b.rowcnt, b.colcnt, b.pos, b.rec, b.d, b.dinv, b.meta);
  perm_scale<T><<<cgrid, EW_THREADS, 0, s>>>(A, lda, Ap, n, n, b.pos, nullptr, nullptr);
  perm_scale<T><<<cgrid, EW_THREADS, 0, s>>>(At, n, Apt, n, n, b.pos, nullptr, nullptr);
  HIPCHECK(hipGetLastError());
  const double tiny = (double)std::numeric_limits<R>::min(), eps = (double)std::numeric_limits<R>::epsilon();
  const double sfmin1 = tiny / eps, sfmax1 = 1.0 / sfmin1, sfmin2 = sfmin1 * 2.0, sfmax2 = 1.0 / sfmin2;
  bal_sweeps<T><<<1, BAL_THREADS, 0, s>>>(Ap, Apt, (int)n, b.d, b.dinv, b.meta, sfmin1, sfmax1, sfmin2, sfmax2);
  bal_factors<<<(unsigned)((n + EW_THREADS - 1) / EW_THREADS), EW_THREADS, 0, s>>>(b.pos, b.d, n, b.inv, b.rf, b.cf, b.urf, b.ucf);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(hmeta, b.meta, sizeof(BalMeta), hipMemcpyDeviceToHost, s));
}
void bal_check_settled(const BalMeta *hmeta) {
  if (hmeta->noconv) fail(EXPV_MI_UNSUPPORTED, "gebal: the scaling loop did not settle in 128 sweeps");
}

template <class T>
void expm_dev(Ctx *ctx, int64_t n, T *A, int64_t lda, int64_t info[8], bool balance) {
  using R = typename ST<T>::real_t;
  constexpr int NP = ST<T>::nreal;
  hipStream_t s = ctx->stream;
  DenseWs *ws = dense_ws(ctx);
  auto need = [&](DevBuf &b, size_t bytes) { if (b.bytes < bytes) b.alloc(bytes); };
  const size_t mat_bytes = ((sizeof(T) * (size_t)n * (size_t)n + 255) / 256) * 256;
  for (auto &w : ws->W) need(w, mat_bytes);
  need(ws->colsum, sizeof(double) * (size_t)n);
  need(ws->ipiv, sizeof(int32_t) * (size_t)n);
  need(ws->stat, sizeof(StatWords));
  if (!ws->pin) HIPCHECK(hipHostMalloc(&ws->pin, sizeof(StatWords), hipHostMallocDefault));
  StatWords *dstat = ws->stat.as<StatWords>(), *hstat = reinterpret_cast<StatWords *>(ws->pin);

  // opnorm(A, 1), column sums in fp64; the norm comes to the host to choose the method, and a non-finite one ends the call here
  HIPCHECK(hipMemsetAsync(dstat, 0, sizeof(StatWords), s));
  colsum_abs<T><<<(unsigned)n, EW_THREADS, 0, s>>>(A, lda, n, ws->colsum.as<double>());
  colsum_max<<<1, EW_THREADS, 0, s>>>(ws->colsum.as<double>(), n, &dstat->norm1);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(hstat, dstat, sizeof(StatWords), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  double nA = hstat->norm1;
  if (!std::isfinite(nA)) fail(EXPV_MI_ARGUMENT_ERROR, "ArgumentError: matrix contains Infs or NaNs");

  // ExpMethodHigham2005Base: balance first, and take the norm AFTER balancing (exp_baseexp.jl:127-129, host_dense.h) -- the one
  // deliberate difference to exp_noalloc.jl:117.  The balanced matrix lands in W[2]; everything below reads it from there.
  const T *src = A;
  int64_t ld_src = lda;
  BalBufs bb{};
  const BalMeta *hmeta = nullptr;
  int64_t bal_us = 0;
  if (balance) {
    const auto t0 = std::chrono::steady_clock::now();
    bb = bal_carve(ws, n);
    hmeta = reinterpret_cast<const BalMeta *>(ws->pinbal);
    T *At = ws->W[1].as<T>(), *Ap = ws->W[2].as<T>(), *Apt = ws->W[3].as<T>();
    balance_dev<T>(ctx, ws, bb, n, A, lda, At, Ap, Apt);
    perm_scale<T><<<column_grid<T>(n), EW_THREADS, 0, s>>>(Ap, n, Ap, n, n, nullptr, bb.rf, bb.cf);
    HIPCHECK(hipMemsetAsync(dstat, 0, sizeof(StatWords), s));
    colsum_abs<T><<<(unsigned)n, EW_THREADS, 0, s>>>(Ap, n, n, ws->colsum.as<double>());
    colsum_max<<<1, EW_THREADS, 0, s>>>(ws->colsum.as<double>(), n, &dstat->norm1);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(hstat, dstat, sizeof(StatWords), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    bal_check_settled(hmeta);
    nA = hstat->norm1;
    if (!std::isfinite(nA)) fail(EXPV_MI_ARGUMENT_ERROR, "ArgumentError: matrix contains Infs or NaNs");
    src = Ap;
    ld_src = n;
    bal_us += (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  }

  const double *Cf;
  int N, si = 0;
  if (nA <= 2.1) {
    if (nA > 0.95) { Cf = dense::PADE_C9; N = 10; }
    else if (nA > 0.25) { Cf = dense::PADE_C7; N = 8; }
    else if (nA > 0.015) { Cf = dense::PADE_C5; N = 6; }
    else { Cf = dense::PADE_C3; N = 4; }
  } else {
    const double l = std::log2(nA / 5.4);
    if (l > 0) si = (int)std::ceil(l);
    Cf = dense::PADE_C13;
    N = 14;
  }

  T *As = ws->W[0].as<T>(), *A2 = ws->W[1].as<T>(), *P = ws->W[2].as<T>(), *tmp = ws->W[3].as<T>(), *U = ws->W[4].as<T>(), *V = ws->W[5].as<T>();
  const T one = host_T<T, double>(1.0, 0.0), zero = host_T<T, double>(0.0, 0.0);
  const int64_t total = n * n * NP;
  const unsigned ew_blocks = (unsigned)std::min<int64_t>((total / Pack<R>::N + EW_THREADS) / EW_THREADS, 4096);
  const dim3 col_grid((unsigned)std::min<int64_t>((n * NP / Pack<R>::N + EW_THREADS) / EW_THREADS, 64), (unsigned)n);
  auto mm = [&](T *Cm, const T *X, const T *Y) { gemm_dev<T>(ctx, n, n, n, one, X, n, Y, n, zero, true, Cm, n); };

  copy_scale<T><<<col_grid, EW_THREADS, 0, s>>>(src, ld_src, As, n, n, (R)std::ldexp(1.0, -si));
  HIPCHECK(hipGetLastError());
  mm(A2, As, As);
  const T *Pk = A2;      // A2^k
  for (int k = 1; k <= N / 2 - 1; ++k) {
    if (k > 1) {
      T *dst = (Pk == P) ? tmp : P;
      mm(dst, Pk, A2);
      Pk = dst;
    }
    horner_update<R><<<ew_blocks, EW_THREADS, 0, s>>>(reinterpret_cast<R *>(U), reinterpret_cast<R *>(V), reinterpret_cast<const R *>(Pk),
                                                     (R)Cf[2 * k + 1], (R)Cf[2 * k], (R)Cf[1], (R)Cf[0], k == 1 ? 1 : 0, total, n, NP);
    HIPCHECK(hipGetLastError());
  }
  T *X = P, *Y = tmp;      // both free again
  mm(X, As, U);           // U <- A U
  sum_diff<R><<<ew_blocks, EW_THREADS, 0, s>>>(reinterpret_cast<R *>(X), reinterpret_cast<R *>(V), total);      // X = V + U, V = V - U
  HIPCHECK(hipGetLastError());
  lu_solve_dev<T>(ctx, n, V, X, ws->ipiv.as<int32_t>(), dstat->lu);
  for (int t = 0; t < si; ++t) {
    mm(Y, X, X);
    std::swap(X, Y);
  }
  // the exchange count and the zero-pivot flag come back together; nothing has touched the caller's matrix yet
  HIPCHECK(hipMemcpyAsync(hstat, dstat, sizeof(StatWords), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  // (dense_force_singular: a host-side seam for the tests -- no finite matrix reaches an exactly zero pivot column)
  if (hstat->lu[1] != 0 || ctx->dense_force_singular) throw dense::SingularError();
  if (!balance) {
    copy_scale<T><<<col_grid, EW_THREADS, 0, s>>>(X, n, A, lda, n, (R)1);
    HIPCHECK(hipGetLastError());
  } else {      // the copy-out IS unbalance: the scaling undone, then the exchanges in reverse (the inverse map), in one pass
    const auto t0 = std::chrono::steady_clock::now();
    perm_scale<T><<<col_grid, EW_THREADS, 0, s>>>(X, n, A, lda, n, hmeta->swaps ? bb.inv : nullptr, bb.urf, bb.ucf);
    HIPCHECK(hipGetLastError());
    if (!ctx->async_out) HIPCHECK(hipStreamSynchronize(s));
    bal_us += (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  }
  if (info) {
    info[0] = N - 1;
    info[1] = si;
    info[2] = hstat->lu[0];
    if (balance) {
      info[4] = hmeta->ilo;
      info[5] = hmeta->ihi;
      info[6] = hmeta->sweeps;
      info[7] = bal_us;
    }
  }
}

template <class T> double norm1_to_host(Ctx *ctx, DenseWs *ws, const T *A, int64_t lda, int64_t n);

// LAPACK.gebal!('B', A) for a device matrix: A balanced in place, ilo / ihi 1-based, scale_host in LAPACK's convention (the factors
// inside ilo .. ihi, 1 + the exchanged position outside).  Complete on return but for the last pass over A (stream-ordered).
template <class T>
void gebal_dev(Ctx *ctx, int64_t n, T *A, int64_t lda, int64_t *ilo, int64_t *ihi, double *scale_host, int64_t *sweeps) {
  hipStream_t s = ctx->stream;
  DenseWs *ws = dense_ws(ctx);
  auto need = [&](DevBuf &b, size_t bytes) { if (b.bytes < bytes) b.alloc(bytes); };
  const size_t mat_bytes = ((sizeof(T) * (size_t)n * (size_t)n + 255) / 256) * 256;
  for (int w = 1; w <= 3; ++w) need(ws->W[w], mat_bytes);
  const double nA = norm1_to_host<T>(ctx, ws, A, lda, n);      // LAPACK.gebal!'s chkfinite
  if (!std::isfinite(nA)) fail(EXPV_MI_ARGUMENT_ERROR, "ArgumentError: matrix contains Infs or NaNs");
  const BalBufs bb = bal_carve(ws, n);
  const BalMeta *hmeta = reinterpret_cast<const BalMeta *>(ws->pinbal);
  T *Ap = ws->W[2].as<T>();
  balance_dev<T>(ctx, ws, bb, n, A, lda, ws->W[1].as<T>(), Ap, ws->W[3].as<T>());
  if (ws->pinscale_bytes < 2 * sizeof(double) * (size_t)n) {
    if (ws->pinscale) (void)hipHostFree(ws->pinscale);
    ws->pinscale = nullptr;
    ws->pinscale_bytes = 0;
    HIPCHECK(hipHostMalloc(&ws->pinscale, 2 * sizeof(double) * (size_t)n, hipHostMallocDefault));
    ws->pinscale_bytes = 2 * sizeof(double) * (size_t)n;
  }
  const double *rec = reinterpret_cast<const double *>(ws->pinscale), *d = rec + n;
  HIPCHECK(hipMemcpyAsync(ws->pinscale, bb.rec, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(reinterpret_cast<double *>(ws->pinscale) + n, bb.d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  bal_check_settled(hmeta);
  perm_scale<T><<<column_grid<T>(n), EW_THREADS, 0, s>>>(Ap, n, A, lda, n, nullptr, bb.rf, bb.cf);
  HIPCHECK(hipGetLastError());
  if (ilo) *ilo = hmeta->ilo;
  if (ihi) *ihi = hmeta->ihi;
  if (sweeps) *sweeps = hmeta->sweeps;
  if (scale_host)
    for (int64_t q = 0; q < n; ++q) scale_host[q] = (q + 1 >= hmeta->ilo && q + 1 <= hmeta->ihi) ? d[q] : rec[q];
}

// ---------------------------------------------------------------------------------------------- phi!(out, A, k)
// phi_0(A) ... phi_k(A) of a device matrix (phi.jl:159-257) by scaling and recovering: s = smallest integer with |A|_1 2^-s <= 1,
// phi_k(As) by its Taylor series to degree M (Paterson-Stockmeyer, tau = 4), phi_j(As) = As phi_{j+1}(As) + I / j! downwards, then s
// times phi_0(2X) = phi_0(X)^2, phi_j(2X) = 2^-j (phi_0(X) phi_j(X) + sum_{i=1..j} phi_i(X) / (j - i)!).  DESIGN.md 4.1.1 derives
// M (18 for the 64-bit types, 10 for the 32-bit ones: the remainder at |As|_1 <= 1 is below the unit roundoff for every k) and
// counts the products: tau - 1 = 3 powers, M / tau Horner steps (4 or 2), k for the recurrence, one WIDE product per recovery step.
constexpr int PHI_MAX_K = 16;
constexpr int PHI_TAU = 4;
static_assert((int64_t)(PHI_MAX_K + 1) * 65535 <= (int64_t)65535 * 64, "grid.y of the wide product: (k + 1) n / 64 at the largest n");

template <class R> struct PhiTab {      // kernel argument of phi_recover: 1 / d! and 2^-j
  R inv_fact[PHI_MAX_K + 1], half_pow[PHI_MAX_K + 1];
};
template <class R> struct One {         // the scalar twin of Pack<R>
  static constexpr int N = 1;
  R v[1];
};

// One recovery step at position i (in units of W) of every block: S_j <- 2^-j (T_j + sum_{i=1..j} S_i / (j - i)!), T = Phi_0 S.
// The old Phi_1 .. Phi_k of the position are held in registers (indices are unrolled constants, j <= k is uniform), then the
// blocks 0 .. k are stored over them.
template <class R, int KM, class W>
__device__ inline void phi_recover_at(R *S, const R *T, int64_t block_words, int64_t i, int k, const PhiTab<R> &tab) {
  W old[KM];
#pragma unroll
  for (int j = 1; j <= KM; ++j)
    if (j <= k) old[j - 1] = reinterpret_cast<const W *>(S + j * block_words)[i];
#pragma unroll
  for (int j = 0; j <= KM; ++j)
    if (j <= k) {
      W acc = reinterpret_cast<const W *>(T + j * block_words)[i];
#pragma unroll
      for (int l = 1; l <= j; ++l)
#pragma unroll
        for (int q = 0; q < W::N; ++q) acc.v[q] += old[l - 1].v[q] * tab.inv_fact[j - l];
#pragma unroll
      for (int q = 0; q < W::N; ++q) acc.v[q] *= tab.half_pow[j];
      reinterpret_cast<W *>(S + j * block_words)[i] = acc;
    }
}
// S and T: slabs of k + 1 packed n x n blocks, seen as block_words real words each.  vec: every block starts on a 16-byte boundary
// (block_words is a multiple of the pack); otherwise the whole pass is scalar.  KM: the compiled register budget, k <= KM.
template <class R, int KM>
__global__ __launch_bounds__(EW_THREADS) void phi_recover(R *S, const R *__restrict__ T, int64_t block_words, int k, PhiTab<R> tab, int vec) {
  const int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * EW_THREADS;
  if (vec) {
    const int64_t np = block_words / Pack<R>::N;
    for (int64_t i = t; i < np; i += nt) phi_recover_at<R, KM, Pack<R>>(S, T, block_words, i, k, tab);
  } else {
    for (int64_t i = t; i < block_words; i += nt) phi_recover_at<R, KM, One<R>>(S, T, block_words, i, k, tab);
  }
}

// Paterson-Stockmeyer block on packed n x n matrices seen as `total` real words: B = c0 I + c1 P1 + c2 P2 + c3 P3 (terms l >= nl
// are not read).  B is the buffer the next Horner product accumulates into (beta = 1).
template <class R>
__global__ __launch_bounds__(EW_THREADS) void ps_block(R *__restrict__ B, const R *__restrict__ P1, const R *__restrict__ P2, const R *__restrict__ P3,
                                                       R c0, R c1, R c2, R c3, int nl, int64_t total, int64_t n, int nreal, int vec) {
  constexpr int N = Pack<R>::N;
  const int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x, nt = (int64_t)gridDim.x * EW_THREADS;
  const int64_t np = vec ? total / N : 0;
  for (int64_t i = t; i < np; i += nt) {
    Pack<R> b;
#pragma unroll
    for (int q = 0; q < N; ++q) b.v[q] = is_diag_real_index(i * N + q, n, nreal) ? c0 : R(0);
    if (nl > 1) {
      const Pack<R> p = reinterpret_cast<const Pack<R> *>(P1)[i];
#pragma unroll
      for (int q = 0; q < N; ++q) b.v[q] += c1 * p.v[q];
    }
    if (nl > 2) {
      const Pack<R> p = reinterpret_cast<const Pack<R> *>(P2)[i];
#pragma unroll
      for (int q = 0; q < N; ++q) b.v[q] += c2 * p.v[q];
    }
    if (nl > 3) {
      const Pack<R> p = reinterpret_cast<const Pack<R> *>(P3)[i];
#pragma unroll
      for (int q = 0; q < N; ++q) b.v[q] += c3 * p.v[q];
    }
    reinterpret_cast<Pack<R> *>(B)[i] = b;
  }
  for (int64_t e = np * N + t; e < total; e += nt) {
    R b = is_diag_real_index(e, n, nreal) ? c0 : R(0);
    if (nl > 1) b += c1 * P1[e];
    if (nl > 2) b += c2 * P2[e];
    if (nl > 3) b += c3 * P3[e];
    B[e] = b;
  }
}

// M[i, i] += d for a packed n x n matrix (the real part, for the complex types)
template <class R>
__global__ __launch_bounds__(EW_THREADS) void add_diag(R *__restrict__ M, int64_t n, int nreal, R d) {
  const int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i < n) M[i * (n + 1) * nreal] += d;
}

template <class R, int KM>
void phi_recover_launch(hipStream_t s, unsigned blocks, R *S, const R *T, int64_t block_words, int k, const PhiTab<R> &tab, int vec) {
  phi_recover<R, KM><<<blocks, EW_THREADS, 0, s>>>(S, T, block_words, k, tab, vec);
}

// opnorm(A, 1) with fp64 column sums, brought to the host (one stream synchronisation); NaN when an entry is not finite
template <class T>
double norm1_to_host(Ctx *ctx, DenseWs *ws, const T *A, int64_t lda, int64_t n) {
  hipStream_t s = ctx->stream;
  auto need = [&](DevBuf &b, size_t bytes) { if (b.bytes < bytes) b.alloc(bytes); };
  need(ws->colsum, sizeof(double) * (size_t)n);
  need(ws->stat, sizeof(StatWords));
  if (!ws->pin) HIPCHECK(hipHostMalloc(&ws->pin, sizeof(StatWords), hipHostMallocDefault));
  StatWords *dstat = ws->stat.as<StatWords>(), *hstat = reinterpret_cast<StatWords *>(ws->pin);
  HIPCHECK(hipMemsetAsync(dstat, 0, sizeof(StatWords), s));
  colsum_abs<T><<<(unsigned)n, EW_THREADS, 0, s>>>(A, lda, n, ws->colsum.as<double>());
  colsum_max<<<1, EW_THREADS, 0, s>>>(ws->colsum.as<double>(), n, &dstat->norm1);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(hstat, dstat, sizeof(StatWords), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return hstat->norm1;
}

// The slab [Phi_0 ... Phi_k] (packed n x n blocks) in the context's workspace; A is only read.  With `out` the blocks are copied to
// out[j] (device, leading dimension ldo) by kernels on the stream; the call itself synchronises once (the norm).
template <class T>
const T *phi_dev(Ctx *ctx, int64_t n, int k, const T *A, int64_t lda, void *const *out, int64_t ldo, int64_t info[8]) {
  using R = typename ST<T>::real_t;
  constexpr int NP = ST<T>::nreal, N = Pack<R>::N;
  hipStream_t s = ctx->stream;
  DenseWs *ws = dense_ws(ctx);
  auto need = [&](DevBuf &b, size_t bytes) { if (b.bytes < bytes) b.alloc(bytes); };
  const size_t mat_bytes = ((sizeof(T) * (size_t)n * (size_t)n + 255) / 256) * 256;
  const size_t slab_bytes = ((sizeof(T) * (size_t)n * (size_t)n * (size_t)(k + 1) + 255) / 256) * 256;
  for (auto &w : ws->W) need(w, mat_bytes);
  need(ws->phiS, slab_bytes);
  need(ws->phiT, slab_bytes);

  const double nA = norm1_to_host<T>(ctx, ws, A, lda, n);
  if (!std::isfinite(nA)) fail(EXPV_MI_ARGUMENT_ERROR, "ArgumentError: matrix contains Infs or NaNs");
  int si = 0;      // the smallest s with nA 2^-s <= theta = 1, from the exponent (no rounding of a logarithm at the thresholds)
  if (nA > 1.0) {
    const double f = std::frexp(nA, &si);      // nA = f 2^si, 0.5 <= f < 1
    if (f == 0.5) --si;
  }
  const int M = sizeof(R) == 8 ? 18 : 10;
  R c[20];      // c[i] = 1 / (i + k)!, i <= M, in fp64, rounded once
  PhiTab<R> tab;
  {
    double f = 1.0;          // d!
    for (int d = 0; d <= PHI_MAX_K; ++d) {
      if (d > 0) f *= d;
      tab.inv_fact[d] = (R)(1.0 / f);
      tab.half_pow[d] = (R)std::ldexp(1.0, -d);
    }
    f = 1.0;
    for (int d = 1; d <= k; ++d) f *= d;
    for (int i = 0; i <= M; ++i) {
      if (i > 0) f *= (i + k);
      c[i] = (R)(1.0 / f);
    }
  }

  T *As = ws->W[0].as<T>(), *P2 = ws->W[1].as<T>(), *P3 = ws->W[2].as<T>(), *P4 = ws->W[3].as<T>(), *X = ws->W[4].as<T>(), *Y = ws->W[5].as<T>();
  T *S = ws->phiS.as<T>(), *Tm = ws->phiT.as<T>();
  const T one = host_T<T, double>(1.0, 0.0), zero = host_T<T, double>(0.0, 0.0);
  const int64_t nn = n * n, total = nn * NP;
  const unsigned ew_blocks = (unsigned)std::min<int64_t>((total / N + EW_THREADS) / EW_THREADS, 4096);
  const dim3 col_grid((unsigned)std::min<int64_t>((n * NP / N + EW_THREADS) / EW_THREADS, 64), (unsigned)n);
  int products = 0;
  auto mm = [&](T *Cm, const T *L, const T *Rt, int64_t ncols, bool accumulate) {
    gemm_dev<T>(ctx, n, ncols, n, one, L, n, Rt, n, accumulate ? one : zero, !accumulate, Cm, n);
    ++products;
  };
  auto is16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };

  copy_scale<T><<<col_grid, EW_THREADS, 0, s>>>(A, lda, As, n, n, (R)std::ldexp(1.0, -si));
  HIPCHECK(hipGetLastError());
  mm(P2, As, As, n, false);
  mm(P3, P2, As, n, false);
  mm(P4, P2, P2, n, false);
  // Horner in As^4 from the top block down; the last step lands in block k of the slab
  T *Sk = S + (int64_t)k * nn;
  const int top = M / PHI_TAU;
  const T *cur = nullptr;
  for (int b = top; b >= 0; --b) {
    T *dst = (b == 0) ? Sk : (cur == X ? Y : X);
    const int nl = std::min(PHI_TAU, M + 1 - b * PHI_TAU);
    const R *cb = c + b * PHI_TAU;
    ps_block<R><<<ew_blocks, EW_THREADS, 0, s>>>(reinterpret_cast<R *>(dst), reinterpret_cast<const R *>(As), reinterpret_cast<const R *>(P2),
                                                reinterpret_cast<const R *>(P3), cb[0], nl > 1 ? cb[1] : R(0), nl > 2 ? cb[2] : R(0),
                                                nl > 3 ? cb[3] : R(0), nl, total, n, NP, is16(dst) ? 1 : 0);
    HIPCHECK(hipGetLastError());
    if (cur) mm(dst, cur, P4, n, true);
    cur = dst;
  }
  // phi_j = As phi_{j+1} + I / j!: the product, then n diagonal entries (a C prefilled with I / j! and beta = 1 would write and
  // read n^2 entries more per step for the same two launches)
  for (int j = k - 1; j >= 0; --j) {
    T *Sj = S + (int64_t)j * nn;
    mm(Sj, As, Sj + nn, n, false);
    add_diag<R><<<(unsigned)((n + EW_THREADS - 1) / EW_THREADS), EW_THREADS, 0, s>>>(reinterpret_cast<R *>(Sj), n, NP, tab.inv_fact[j]);
    HIPCHECK(hipGetLastError());
  }
  // recovery: one wide product T = Phi_0 [Phi_0 ... Phi_k], one element-wise pass over both slabs
  const int vec = (total % N == 0) ? 1 : 0;
  const unsigned rec_blocks = (unsigned)std::min<int64_t>(((vec ? total / N : total) + EW_THREADS - 1) / EW_THREADS, 8192);
  for (int t = 0; t < si; ++t) {
    mm(Tm, S, S, (int64_t)(k + 1) * n, false);
    ProfScope ps(ctx, EXPV_MI_K_LINCOMB);      // (expv_mi_prof_get: the recovery pass is timed under "lincomb", tools/phi_device.py)
    R *Sr = reinterpret_cast<R *>(S);
    const R *Tr = reinterpret_cast<const R *>(Tm);
    if (k <= 1) phi_recover_launch<R, 1>(s, rec_blocks, Sr, Tr, total, k, tab, vec);
    else if (k <= 2) phi_recover_launch<R, 2>(s, rec_blocks, Sr, Tr, total, k, tab, vec);
    else if (k <= 4) phi_recover_launch<R, 4>(s, rec_blocks, Sr, Tr, total, k, tab, vec);
    else if (k <= 8) phi_recover_launch<R, 8>(s, rec_blocks, Sr, Tr, total, k, tab, vec);
    else phi_recover_launch<R, PHI_MAX_K>(s, rec_blocks, Sr, Tr, total, k, tab, vec);
    HIPCHECK(hipGetLastError());
  }
  if (out) {
    for (int j = 0; j <= k; ++j) copy_scale<T><<<col_grid, EW_THREADS, 0, s>>>(S + (int64_t)j * nn, n, reinterpret_cast<T *>(out[j]), ldo, n, (R)1);
    HIPCHECK(hipGetLastError());
  }
  if (info) {
    info[0] = M;
    info[1] = si;
    info[2] = products;
  }
  return S;
}

}  // namespace

int dense_phi_max_k() { return PHI_MAX_K; }

const void *dense_phi_run(Ctx *ctx, int dtype, int64_t n, int k, const void *A_dev, int64_t lda, void *const *out_dev, int64_t ldo,
                          int64_t info[8]) {
  const void *slab = nullptr;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    slab = phi_dev<T>(ctx, n, k, reinterpret_cast<const T *>(A_dev), lda, out_dev, ldo, info);
  });
  return slab;
}

void dense_gemm_run(Ctx *ctx, int dtype, int64_t m, int64_t n, int64_t k, double alpha_re, double alpha_im, const void *A, int64_t lda,
                    const void *B, int64_t ldb, double beta_re, double beta_im, void *C, int64_t ldc) {
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    gemm_dev<T>(ctx, m, n, k, host_T<T, double>(alpha_re, alpha_im), reinterpret_cast<const T *>(A), lda, reinterpret_cast<const T *>(B), ldb,
                host_T<T, double>(beta_re, beta_im), beta_re == 0.0 && beta_im == 0.0, reinterpret_cast<T *>(C), ldc);
  });
}

void dense_expm_run(Ctx *ctx, int dtype, int64_t n, void *A_dev, int64_t lda, int64_t info[8], bool balance) {
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    expm_dev<T>(ctx, n, reinterpret_cast<T *>(A_dev), lda, info, balance);
  });
}

void dense_gebal_run(Ctx *ctx, int dtype, int64_t n, void *A_dev, int64_t lda, int64_t *ilo, int64_t *ihi, double *scale_host, int64_t *sweeps) {
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    gebal_dev<T>(ctx, n, reinterpret_cast<T *>(A_dev), lda, ilo, ihi, scale_host, sweeps);
  });
}

}  // namespace expv_mi
