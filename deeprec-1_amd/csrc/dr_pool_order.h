// dr_pool_order.h -- the reference association order of a pooled bag
// (DR_ORDER_ALI: SparseSegmentReduction::Reduce,
// core/kernels/segment_reduction_ali_ops_util.h:193-318, and the weighted
// composition of python/ops/embedding_ops.py:609-651) over an abstract row
// source: Fill(x, k) fills the Row x with the row of bag position k, so a row
// may be fetched from one table (pool.hip: a row pointer, clipped by max_norm)
// or combined from several (multihash.hip).  The order exists here once; both
// files pool through it.
#pragma once
#include "dr_common.h"
#include "dr_rows.h"

namespace dr {

// Unweighted bag of `num` >= 1 rows -> acc, in the ALI order:
//  * num == 1: the row itself (a copy, no add);
//  * a first chunk of num % 8 rows (0 -> 8, 1 -> 9) summed left to right;
//  * mean / sqrtn divide that first chunk when num < 10 ...
//  * then chunks of 8, each summed left to right and added to acc;
//  * ... and divide the total when num >= 10.
template <int VEC, int G, int CPL, class Fill>
__device__ __forceinline__ void ali_bag_rows(Row<VEC, G, CPL>& acc, int64_t num, int combiner,
                                             const Fill& F) {
  using R = Row<VEC, G, CPL>;
  if (num == 1) {
    F(acc, (int64_t)0);
    return;
  }
  int64_t r = num % 8;
  if (r == 0) r = 8;
  if (r == 1) r = 9;
  {
    R x[9];
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (j < r) F(x[j], (int64_t)j);
    acc = x[0];
#pragma unroll
    for (int j = 1; j < 9; ++j)
      if (j < r) acc_add(acc, x[j]);
  }
  if (num < 10 && combiner != DR_COMBINER_SUM) {
    const float m = combiner == DR_COMBINER_MEAN ? (float)num : (float)sqrt((double)num);
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc.v[c] = vdiv(acc.v[c], m);
  }
  for (int64_t g = r; g < num; g += 8) {
    R x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) F(x[j], g + j);
    R s = x[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) acc_add(s, x[j]);
    acc_add(acc, s);
  }
  if (num >= 10 && combiner != DR_COMBINER_SUM) {
    const float q = combiner == DR_COMBINER_MEAN ? (float)num : (float)sqrt((double)num);
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc.v[c] = vdiv(acc.v[c], q);
  }
}

// Weighted bag (w[k] = weight of position k, num >= 0; either pooling order):
// acc = sum row * w left to right from 0, divided by sum(w) (mean) or
// sqrt(sum(w^2)) (sqrtn).  An empty mean / sqrtn bag is 0 / 0 = NaN, as the
// reference's.
template <int VEC, int G, int CPL, class Fill>
__device__ __forceinline__ void bag_rows_weighted(Row<VEC, G, CPL>& acc, int64_t num,
                                                      int combiner, const float* w,
                                                      const Fill& F) {
  using R = Row<VEC, G, CPL>;
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc.v[c] = vzero<typename VecT<VEC>::T>();
  float wsum = 0.f;
  for (int64_t k = 0; k < num; ++k) {
    R x;
    F(x, k);
    const float wk = gld(w + k);
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc.v[c] = vadd(acc.v[c], vmul(x.v[c], wk));
    wsum = wsum + (combiner == DR_COMBINER_SQRTN ? wk * wk : wk);
  }
  if (combiner != DR_COMBINER_SUM) {
    const float q = combiner == DR_COMBINER_SQRTN ? sqrtf(wsum) : wsum;
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc.v[c] = vdiv(acc.v[c], q);
  }
}

// The empty-bag rule: an empty bag is a zero row -- except with weights and
// mean / sqrtn, where the reference divides the zero segment_sum by a zero
// weight sum (embedding_ops.py:636-645): 0 / 0 = NaN, which the weighted order
// above reproduces.
__device__ __forceinline__ bool bag_is_zero(int64_t num, const float* w, int combiner) {
  return num <= 0 && !(w && combiner != DR_COMBINER_SUM);
}

// One whole bag: the empty-bag rule, then one of the two orders above.
template <int VEC, int G, int CPL, class Fill>
__device__ __forceinline__ void ali_bag(Row<VEC, G, CPL>& acc, int64_t num, int combiner,
                                        const float* w, const Fill& F) {
  if (bag_is_zero(num, w, combiner)) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc.v[c] = vzero<typename VecT<VEC>::T>();
    return;
  }
  if (w)
    bag_rows_weighted<VEC, G, CPL>(acc, num, combiner, w, F);
  else
    ali_bag_rows<VEC, G, CPL>(acc, num, combiner, F);
}

}  // namespace dr
