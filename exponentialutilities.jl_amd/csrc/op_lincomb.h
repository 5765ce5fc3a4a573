// op_lincomb.h -- launchers of op_lincomb.hip: C = c_1 A_1 + ... + c_K A_K (+ c_I I) of operators that exist, made on the device
// from what they store (capi.hip: expv_mi_op_create_lincomb, expv_mi_op_lincomb_refresh).
#pragma once
#include <cstdint>

#include "device_types.h"

namespace expv_mi {
namespace dev {

constexpr int LINCOMB_MAX_TERMS = 8;      // EXPV_MI_LINCOMB_MAX_TERMS (include/expv_mi.h; capi.hip asserts that the two agree)

// What the two value kernels take BY VALUE, in the kernel arguments: the terms' value arrays, where each term's entries start in the
// concatenation of the terms' stored arrays, and the coefficients, rounded once to the element type's real type.  Slot `nterms`
// of the coefficients is the identity's.
template <class T>
struct LincombTerms {
  using R = typename ST<T>::real_t;
  const T *val[LINCOMB_MAX_TERMS];        // sparse: the term's stored values; dense: its column-major matrix
  int64_t lda[LINCOMB_MAX_TERMS];         // dense: the term's leading dimension (sparse: unused)
  // sparse: off[k] = first position of term k, off[nterms] = sum of the terms' nnz (where the identity's n entries start);
  // off[k] = INT32_MAX for k > nterms, so that counting the offsets <= g gives the term of position g
  int32_t off[LINCOMB_MAX_TERMS + 1];
  R cre[LINCOMB_MAX_TERMS + 1], cim[LINCOMB_MAX_TERMS + 1];
  int nterms, identity;
};

int lincomb_pack(int value_bytes);       // output entries a lane of the gather-scale-sum owns (one 16-byte store)
// the term's stored CSR32 arrays (p: its row ordering, position -> natural row; null: natural) -> key[base + e] =
// p[row] << 32 | p[col] of stored entry e and pay[base + e] = base + e
void lincomb_keys(hipStream_t s, const int32_t *rowptr, const int32_t *col, const int32_t *p, int64_t n, int64_t nnz, int64_t base,
                  unsigned long long *key, int32_t *pay);
// key[base + i] = i << 32 | i, pay[base + i] = base + i, i < n: the identity's entries
void lincomb_identity_keys(hipStream_t s, int64_t n, int64_t base, unsigned long long *key, int32_t *pay);
// out[e] = sum over q = seg[e] .. seg[e + 1] - 1 of c_t val_t[src[q] - off[t]], t the term of position src[q], left to right, the
// accumulator starting as the first contribution (out 16-byte aligned; every segment holds one position at least)
template <class T>
void lincomb_gather(hipStream_t s, const LincombTerms<T> &a, const int32_t *src, const int32_t *seg, int64_t nstored, T *out);
// out[i + j n] = c_1 A_1[i + j lda_1] + ... (+ c_I where i == j), i, j < n, left to right; rows n .. lda - 1 of a term are not read
template <class T>
void lincomb_dense(hipStream_t s, const LincombTerms<T> &a, int64_t n, T *out);

}  // namespace dev
}  // namespace expv_mi
