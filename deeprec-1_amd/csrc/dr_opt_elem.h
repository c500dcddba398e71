// dr_opt_elem.h -- the sparse optimizers' scalars and per-element updates,
// shared by the EV apply kernels (ev.hip) and the dense-table apply
// (dense_apply.hip): one definition of every formula, so a dense table and an
// EmbeddingVariable holding the same rows take bit-identical steps.  Every
// element is the reference's scalar formula with separate fp32 roundings
// (built with -ffp-contract=off).
#pragma once
#include "dr_common.h"

namespace dr {

enum {
  OPT_SGD = 0,
  OPT_ADAGRAD = 1,
  OPT_ADAM = 2,
  OPT_FTRL = 3,
  OPT_ADAM_ASYNC = 4,     // KvSparseApplyAdamAsync (training_ali_ops.cc:1404-1575)
  OPT_ADAM_RMSPROP = 5,   //   ... with apply_sparse_rmsprop (:1483-1519)
  OPT_ADAGRAD_DECAY = 6   // KvSparseApplyAdagradDecay (training_ali_ops.cc:703-823)
};
// var + two slot columns (m / v, or accum / accum_decay_power)
__host__ __device__ constexpr bool opt_three_cols(int opt) {
  return opt == OPT_ADAM || opt == OPT_ADAM_ASYNC || opt == OPT_ADAM_RMSPROP ||
         opt == OPT_ADAGRAD_DECAY;
}

struct OptScalars {
  float lr, beta1, beta2, eps, alpha;
  float l1, l2, lr_power, l2_shrinkage;  // FTRL
  float decay_rate, decay_baseline;      // AdagradDecay
  int64_t decay_step;
};

template <int OPT, int VEC, int G>
__device__ __forceinline__ float apply_one(float gv, float w, float* a1, float* a2,
                                           const OptScalars& sc) {
  if (OPT == OPT_SGD) {
    const float p = sc.lr * gv;  // v -= lr * g  (training_ali_ops.cc:1663)
    return w - p;
  } else if (OPT == OPT_ADAGRAD) {  // training_ali_ops.cc:131-132
    float a = *a1;
    const float g2 = gv * gv;
    a = a + g2;
    const float lg_ = sc.lr * gv;
    const float rs = 1.0f / sqrtf(a);
    const float up = lg_ * rs;
    *a1 = a;
    return w - up;
  } else if (OPT == OPT_ADAM_ASYNC) {  // training_ali_ops.cc:1552-1554
    float m = *a1;
    float v = *a2;
    const float mt = m * sc.beta1;
    const float mg = gv * (1.0f - sc.beta1);
    m = mt + mg;
    const float vt = v * sc.beta2;
    const float g2 = gv * gv;
    const float vg = g2 * (1.0f - sc.beta2);
    v = vt + vg;
    const float num = m * sc.alpha;
    const float den = sqrtf(v) + sc.eps;
    *a1 = m;
    *a2 = v;
    return w - num / den;
  } else if (OPT == OPT_ADAM_RMSPROP) {  // training_ali_ops.cc:1506-1513
    float m = *a1;
    float v = *a2;
    const float vt = v * sc.beta2;
    const float g2 = gv * gv;
    const float vg = g2 * (1.0f - sc.beta2);
    v = vt + vg;
    const float rs = 1.0f / sqrtf(v + sc.eps);
    const float step = (rs * sc.lr) * gv;
    const float mt = m * sc.beta1;
    m = mt + step;
    *a1 = m;
    *a2 = v;
    return w - m;
  } else {  // OPT_ADAM, training_ali_ops.cc:952-958
    float m = *a1;
    float v = *a2;
    float t1 = gv - m;
    t1 = t1 * (1.0f - sc.beta1);
    m = m + t1;
    float t2 = gv * gv;
    t2 = t2 - v;
    t2 = t2 * (1.0f - sc.beta2);
    v = v + t2;
    const float num = m * sc.alpha;
    const float den = sqrtf(v) + sc.eps;
    *a1 = m;
    *a2 = v;
    return w - num / den;
  }
}

// AdagradDecay element (training_ali_ops.cc:802-808): when the row decays
// this step, a = max(a * rate, baseline) (cwiseMax: a < b ? b : a), then
// a += g^2; v -= (lr * g) * rsqrt(a).
__device__ __forceinline__ float adagrad_decay_one(float gv, float w, float* a1, bool dec,
                                                   const OptScalars& sc) {
  float a = *a1;
  if (dec) {
    a = a * sc.decay_rate;
    a = a < sc.decay_baseline ? sc.decay_baseline : a;
  }
  const float g2 = gv * gv;
  a = a + g2;
  const float lg_ = sc.lr * gv;
  const float rs = 1.0f / sqrtf(a);
  const float up = lg_ * rs;
  *a1 = a;
  return w - up;
}

// Dense FTRL element (ResourceSparseApplyFtrl[V2], training_ops.cc:2587-2614):
// elementwise, the clip is on the element's own linear (the KV op's row norm
// is ev_apply_ftrl_kernel's).  g is the row's summed gradient; accum takes the
// plain g, linear the shrunk one (V2).  P(x) = sqrt(x) when lr_power == -0.5,
// else x^(-lr_power) (ftrl_pow's selection).
__device__ __forceinline__ float ftrl_dense_one(float gv, float w, float* a1, float* a2,
                                                const OptScalars& sc) {
  const float a = *a1;
  float lin = *a2;
  float gu = gv;
  if (sc.l2_shrinkage > 0.0f) {
    const float sh = (2.0f * sc.l2_shrinkage) * w;
    gu = gv + sh;
  }
  const float g2 = gv * gv;
  const float na = a + g2;
  const bool root = sc.lr_power == -0.5f;
  const float pn = root ? sqrtf(na) : powf(na, -sc.lr_power);
  const float po = root ? sqrtf(a) : powf(a, -sc.lr_power);
  const float dp = pn - po;
  const float q = dp / sc.lr;
  const float t = q * w;
  const float d = gu - t;
  lin = lin + d;
  const float y0 = pn / sc.lr;
  const float y = y0 + 2.0f * sc.l2;
  float c = lin < -sc.l1 ? -sc.l1 : lin;   // min(max(lin, -l1), l1); a NaN stays
  c = c > sc.l1 ? sc.l1 : c;
  const float num = c - lin;
  *a1 = na;
  *a2 = lin;
  return num / y;
}

// Dense Adam (adam.py _apply_sparse_shared, TF's non-lazy sparse Adam) on a
// row no gradient names: m and v decay and the row still moves.  Nothing is
// added to m (m * beta1 + 0.0f would turn a -0.0 into +0.0).  A named row
// takes apply_one<OPT_ADAM_ASYNC>, the same arithmetic with the gradient in.
__device__ __forceinline__ float adam_unnamed_one(float w, float* a1, float* a2,
                                                  const OptScalars& sc) {
  const float m = *a1 * sc.beta1;
  const float v = *a2 * sc.beta2;
  const float num = m * sc.alpha;
  const float den = sqrtf(v) + sc.eps;
  *a1 = m;
  *a2 = v;
  return w - num / den;
}

}  // namespace dr
