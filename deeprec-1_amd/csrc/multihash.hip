// multihash.hip -- MultiHashVariable ("Q-R"): fused lookup + pooling over the
// rows combined from two small tables, the unpooled lookup, and the split of
// the per-unique-id gradient into the two tables' IndexedSlices.
//
// The tables are the re-used data (a Q-R pair of a 12.5 M id feature is two
// 1.8 MB tables: cache resident), so their rows are read with the default
// cache policy; the one-hot output is written once, nontemporal, like
// pool.hip's one-hot copy.  Row layout (VEC / G / CPL) and the row helpers
// are dr_rows.h's; the pooled association order is dr_pool_order.h's.
// Row loads use always-valid pointers (an out-of-range q is clamped, the row
// discarded after the load: load_row_u's reason), never a branch per load.
#include <algorithm>

#include "dr_common.h"
#include "dr_multihash.h"
#include "dr_pool_order.h"
#include "dr_rows.h"

namespace dr {

// One pooled sub-lookup as the kernels see it.  add / mul features are one
// sub-lookup over both tables; a concat feature is two, of Q by q and of R by
// r, each at its own column of the output rows.
enum { MHV_ADD = DR_MHV_ADD, MHV_MUL = DR_MHV_MUL, MHV_Q = 2, MHV_R = 3 };
struct MhvSub {
  const float* qt;
  const float* rt;
  int64_t q_rows, r_rows;
  const int64_t* ids;
  const int32_t* bag_off;
  const float* weights;
  float* out;
  int64_t out_stride;
  int32_t combiner;
  int32_t kind;
};
struct MhvArgs {
  MhvSub d[DR_MAX_GROUP];
};

__device__ __forceinline__ float4 vmulv(float4 a, float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float vmulv(float a, float b) { return a * b; }

// The combined row of nnz position k.  TWO: add / mul (both tables, `dim`
// columns each); else one table's row (concat halves).  live == false: a
// padding slot -- loads an in-bounds row that the caller drops, latches
// nothing.
template <int VEC, int G, int CPL, bool TWO>
__device__ __forceinline__ void mhv_fetch(Row<VEC, G, CPL>& x, const MhvSub& d, int64_t k,
                                          int dim, int lg, int dv, int* st, bool live = true) {
  using V = typename VecT<VEC>::T;
  const int64_t id = gld(d.ids + k);
  int64_t q, r;
  dr_mhv_index(id, d.q_rows, d.r_rows, &q, &r);
  const bool ok = dr_mhv_q_valid(q, d.q_rows);
  const int64_t qc = ok ? q : 0;
  if constexpr (TWO) {
    Row<VEC, G, CPL> a, b;
    load_row_u<VEC, G, CPL>(a, d.qt + qc * (int64_t)dim, lg, dv);
    load_row_u<VEC, G, CPL>(b, d.rt + r * (int64_t)dim, lg, dv);
    const bool mul = d.kind == MHV_MUL;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      // one fp32 operation per element (built with -ffp-contract=off: no FMA
      // with the pooling adds or the weight multiply that follow)
      const V s = vadd(a.v[c], b.v[c]), p = vmulv(a.v[c], b.v[c]);
      x.v[c] = mul ? p : s;
    }
  } else {
    const float* p = d.kind == MHV_Q ? d.qt + qc * (int64_t)dim : d.rt + r * (int64_t)dim;
    load_row_u<VEC, G, CPL>(x, p, lg, dv);
  }
  // as an out-of-range id of a dense table (pool.hip select_row): a zero row
  if (!ok && live) latch(st, DR_INVALID_ARGUMENT);
#pragma unroll
  for (int c = 0; c < CPL; ++c) x.v[c] = ok ? x.v[c] : vzero<V>();
}

// One-hot (bag b is nnz b) in OUTPUT order, as pool.hip's pool_onehot_kernel:
// group g covers slots g*NB .. g*NB+NB-1 of the [B, T] slot grid.  Also the
// unpooled lookup (T = 1, B = n ids; n_dev: device count of the ids, rows past
// it are not written).
template <int VEC, int G, int CPL, bool TWO, int NB>
__global__ __launch_bounds__(256) void mhv_onehot_kernel(MhvArgs args, int T, int64_t B,
                                                         const int64_t* __restrict__ n_dev,
                                                         int dim, int* st) {
  __shared__ MhvSub sd[DR_MAX_GROUP];  // per-lane table index: stage in LDS
  if (threadIdx.x < T) sd[threadIdx.x] = args.d[threadIdx.x];
  __syncthreads();
  constexpr int GPB = 256 / G;
  const int64_t slots = (int64_t)T * B;
  const int64_t s0 = ((int64_t)blockIdx.x * GPB + threadIdx.x / G) * NB;
  if (s0 >= slots) return;
  const int64_t Be = eff_n(B, n_dev);
  const int lg = threadIdx.x % G;
  const int dv = dim / VEC;
  Row<VEC, G, CPL> x[NB];
  float* o[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int64_t s = s0 + j;
    // slots < 2^31 (checked on the host): 32-bit division
    int64_t b = (int64_t)((uint32_t)s / (uint32_t)T);
    int t = (int)(s - b * T);
    const bool live = s < slots && b < Be;
    if (!live) b = 0, t = 0;  // (B >= 1: ids[0] exists)
    const MhvSub& d = sd[t];
    mhv_fetch<VEC, G, CPL, TWO>(x[j], d, b, dim, lg, dv, st, live);
    o[j] = live ? d.out + b * d.out_stride : nullptr;
  }
  wait_loads();
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (o[j]) store_row_nt<VEC, G, CPL>(x[j], o[j], lg, dv);
}

// One bag per lane group over a capped grid that strides through the bags
// (pool.hip's pool_general_kernel), any bag length, weights or not.
template <int VEC, int G, int CPL, bool TWO>
__global__ __launch_bounds__(256) void mhv_bags_kernel(MhvArgs args, int T, int64_t B, int dim,
                                                       int* st) {
  __shared__ MhvSub sd[DR_MAX_GROUP];
  if (threadIdx.x < T) sd[threadIdx.x] = args.d[threadIdx.x];
  __syncthreads();
  constexpr int GPB = 256 / G;
  const int lg = threadIdx.x % G;
  const int dv = dim / VEC;
  const int64_t total = (int64_t)T * B;
  for (int64_t item = (int64_t)blockIdx.x * GPB + threadIdx.x / G; item < total;
       item += (int64_t)gridDim.x * GPB) {
    const int t = (int)(item / B);
    const int64_t b = item - (int64_t)t * B;
    const MhvSub& d = sd[t];
    const int64_t k0 = gld(d.bag_off + b);
    const int64_t num = (int64_t)gld(d.bag_off + b + 1) - k0;
    Row<VEC, G, CPL> acc;
    ali_bag<VEC, G, CPL>(acc, num, d.combiner, d.weights ? d.weights + k0 : nullptr,
                         [&](Row<VEC, G, CPL>& x, int64_t k) {
                           mhv_fetch<VEC, G, CPL, TWO>(x, d, k0 + k, dim, lg, dv, st);
                         });
    store_row<VEC, G, CPL>(acc, d.out + b * d.out_stride, lg, dv);
  }
}

static constexpr int kMhvOneHotNB = 4;                  // rows in flight per lane group
static constexpr int64_t kMhvBagBlocks = 256 * 16;      // bags-kernel grid cap (16 per CU)

template <int VEC, int G, int CPL, bool TWO>
static int launch_mhv(const MhvArgs& a, int T, int64_t B, const int64_t* n_dev, int dim,
                      bool onehot, hipStream_t s, int* st) {
  if (onehot) {
    const int64_t items = ceil_div((int64_t)T * B, kMhvOneHotNB);
    hipLaunchKernelGGL((mhv_onehot_kernel<VEC, G, CPL, TWO, kMhvOneHotNB>),
                       dim3((unsigned)ceil_div(items, 256 / G)), dim3(256), 0, s, a, T, B, n_dev,
                       dim, st);
  } else {
    const int64_t blocks = std::min<int64_t>(ceil_div((int64_t)T * B, 256 / G), kMhvBagBlocks);
    hipLaunchKernelGGL((mhv_bags_kernel<VEC, G, CPL, TWO>), dim3((unsigned)blocks), dim3(256), 0,
                       s, a, T, B, dim, st);
  }
  DR_LAUNCH_CHECK();
  return DR_OK;
}

// The row shapes dispatch_pool<DR_ORDER_ALI> (pool.hip) accepts for fp32.
static bool mhv_dim_ok(int dim, bool v4) { return dim >= 1 && dim <= (v4 ? 1024 : 256); }

template <bool TWO>
static int dispatch_mhv(const MhvArgs& a, int T, int64_t B, const int64_t* n_dev, int dim, bool v4,
                        bool onehot, hipStream_t s, int* st) {
#define DR_MHV(V, G, C) return launch_mhv<V, G, C, TWO>(a, T, B, n_dev, dim, onehot, s, st)
  if (v4) {
    const int d4 = dim / 4;
    if (d4 <= 1) DR_MHV(4, 1, 1);
    if (d4 <= 2) DR_MHV(4, 2, 1);
    if (d4 <= 4) DR_MHV(4, 4, 1);
    if (d4 <= 8) DR_MHV(4, 8, 1);
    if (d4 <= 16) DR_MHV(4, 16, 1);
    if (d4 <= 32) DR_MHV(4, 32, 1);
    if (d4 <= 64) DR_MHV(4, 64, 1);
    if (d4 <= 128) DR_MHV(4, 64, 2);
    if (d4 <= 256) DR_MHV(4, 64, 4);
  } else {
    if (dim <= 4) DR_MHV(1, 4, 1);
    if (dim <= 8) DR_MHV(1, 8, 1);
    if (dim <= 16) DR_MHV(1, 16, 1);
    if (dim <= 32) DR_MHV(1, 32, 1);
    if (dim <= 64) DR_MHV(1, 64, 1);
    if (dim <= 256) DR_MHV(1, 64, 4);
  }
#undef DR_MHV
  set_error("multihash: row width %d unsupported", dim);
  return DR_INVALID_ARGUMENT;
}

// A sub-lookup with the launch it belongs to: sub-lookups of equal width,
// vector width, table count and one-hot-ness share launches.
struct MhvPlan {
  MhvSub sub;
  int dim;
  bool v4, two, onehot;
  bool same_launch(const MhvPlan& o) const {
    return dim == o.dim && v4 == o.v4 && two == o.two && onehot == o.onehot;
  }
};

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Validates the descriptors and expands them into sub-lookups (<= 2 each).
// Nothing is launched here.
static int plan_mhv(const dr_mhv_desc* descs, int num_tables, int64_t batch, MhvPlan* plans,
                    int* num_plans) {
  DR_REQUIRE(descs, DR_INVALID_ARGUMENT, "multihash: null descriptors");
  DR_REQUIRE(num_tables >= 1 && num_tables <= DR_MAX_GROUP, DR_INVALID_ARGUMENT,
             "multihash: num_tables must be in [1, %d]", DR_MAX_GROUP);
  DR_REQUIRE(batch >= 0, DR_INVALID_ARGUMENT, "multihash: negative batch");
  int n = 0;
  for (int t = 0; t < num_tables; ++t) {
    const dr_mhv_desc& d = descs[t];
    DR_REQUIRE(d.q_table && d.r_table && d.ids && d.out, DR_INVALID_ARGUMENT,
               "multihash feature %d: null table, ids or out", t);
    DR_REQUIRE(d.q_rows >= 1 && d.r_rows >= 1 && d.q_dim >= 1 && d.r_dim >= 1,
               DR_INVALID_ARGUMENT, "multihash feature %d: rows and dims must be >= 1", t);
    DR_REQUIRE(d.operation == DR_MHV_ADD || d.operation == DR_MHV_MUL ||
                   d.operation == DR_MHV_CONCAT,
               DR_INVALID_ARGUMENT, "multihash feature %d: unknown operation %d", t, d.operation);
    DR_REQUIRE(d.operation == DR_MHV_CONCAT || d.q_dim == d.r_dim, DR_INVALID_ARGUMENT,
               "multihash feature %d: add / mul need q_dim == r_dim (%d vs %d)", t, d.q_dim,
               d.r_dim);
    DR_REQUIRE(d.combiner == DR_COMBINER_SUM || d.combiner == DR_COMBINER_MEAN ||
                   d.combiner == DR_COMBINER_SQRTN,
               DR_INVALID_ARGUMENT, "multihash feature %d: unknown combiner %d", t, d.combiner);
    DR_REQUIRE(d.bag_off || !d.weights, DR_INVALID_ARGUMENT,
               "multihash feature %d: one-hot (no bag_off) excludes weights", t);
    const int64_t width =
        d.operation == DR_MHV_CONCAT ? (int64_t)d.q_dim + d.r_dim : (int64_t)d.q_dim;
    DR_REQUIRE(d.out_stride >= width, DR_INVALID_ARGUMENT,
               "multihash feature %d: out_stride %lld < %lld columns", t, (long long)d.out_stride,
               (long long)width);
    const int parts = d.operation == DR_MHV_CONCAT ? 2 : 1;
    for (int h = 0; h < parts; ++h) {
      MhvPlan& p = plans[n++];
      p.sub.qt = d.q_table;
      p.sub.rt = d.r_table;
      p.sub.q_rows = d.q_rows;
      p.sub.r_rows = d.r_rows;
      p.sub.ids = d.ids;
      p.sub.bag_off = d.bag_off;
      p.sub.weights = d.weights;
      p.sub.out = d.out + (h ? d.q_dim : 0);
      p.sub.out_stride = d.out_stride;
      p.sub.combiner = d.combiner;
      p.sub.kind = parts == 2 ? (h ? MHV_R : MHV_Q) : d.operation;
      p.dim = h ? d.r_dim : d.q_dim;
      p.two = parts == 1;
      p.onehot = d.bag_off == nullptr;
      const bool tabs = p.two ? aligned16(d.q_table) && aligned16(d.r_table)
                              : aligned16(h ? d.r_table : d.q_table);
      p.v4 = p.dim % 4 == 0 && tabs && aligned16(p.sub.out) && d.out_stride % 4 == 0;
      DR_REQUIRE(mhv_dim_ok(p.dim, p.v4), DR_INVALID_ARGUMENT,
                 "multihash feature %d: row width %d unsupported (max 1024 when a multiple of 4 "
                 "and 16-byte aligned, else 256)", t, p.dim);
    }
  }
  *num_plans = n;
  return DR_OK;
}

static int run_mhv(const dr_mhv_desc* descs, int num_tables, int64_t batch, const int64_t* n_dev,
                   hipStream_t s) {
  MhvPlan plans[2 * DR_MAX_GROUP];
  int n = 0;
  int rc = plan_mhv(descs, num_tables, batch, plans, &n);
  if (rc) return rc;
  bool done[2 * DR_MAX_GROUP] = {};
  // (one-hot slots are divided in 32 bits)
  int nh = 0;
  for (int i = 0; i < n; ++i) nh += plans[i].onehot;
  nh = std::min(nh, DR_MAX_GROUP);
  DR_REQUIRE((int64_t)nh * batch < (1ll << 31), DR_INVALID_ARGUMENT,
             "multihash: one-hot needs tables x batch < 2^31");
  if (batch == 0) return DR_OK;
  int* st = status_word();
  DR_REQUIRE(st, DR_INTERNAL, "status word unavailable");
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    MhvArgs a;
    memset(&a, 0, sizeof(a));
    int T = 0;
    for (int j = i; j < n && T < DR_MAX_GROUP; ++j) {
      if (done[j] || !plans[j].same_launch(plans[i])) continue;
      a.d[T++] = plans[j].sub;
      done[j] = true;
    }
    const MhvPlan& p = plans[i];
    rc = p.two ? dispatch_mhv<true>(a, T, batch, n_dev, p.dim, p.v4, p.onehot, s, st)
               : dispatch_mhv<false>(a, T, batch, n_dev, p.dim, p.v4, p.onehot, s, st);
    if (rc) return rc;
  }
  return DR_OK;
}

// Gradient split.  A row of W = (concat ? dvq + dvr : dvq) vector columns per
// unique id; a block covers 256 >> shift ids with 1 << shift lanes each.
template <int VEC>
__global__ __launch_bounds__(256) void mhv_grad_kernel(
    const float* __restrict__ qt, int64_t q_rows, int q_dim, const float* __restrict__ rt,
    int64_t r_rows, int r_dim, int op, const int64_t* __restrict__ uniq,
    const float* __restrict__ gu, int64_t n, const int64_t* __restrict__ n_dev,
    int64_t* __restrict__ q_idx, int64_t* __restrict__ r_idx, float* q_val, float* r_val,
    int shift) {
  using V = typename VecT<VEC>::T;
  const int lanes = 1 << shift;
  const int col0 = threadIdx.x & (lanes - 1);
  const int64_t i = (int64_t)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
  if (i >= n) return;
  const int dvq = q_dim / VEC, dvr = r_dim / VEC;
  const bool cat = op == DR_MHV_CONCAT;
  const int W = cat ? dvq + dvr : dvq;
  const int dim = cat ? q_dim + r_dim : q_dim;
  int64_t q = -1, r = -1;
  bool ok = false;
  if (i < eff_n(n, n_dev)) {
    dr_mhv_index(gld(uniq + i), q_rows, r_rows, &q, &r);
    ok = dr_mhv_q_valid(q, q_rows);
  }
  const int64_t qc = ok ? q : 0, rc = ok ? r : 0;
  if (col0 == 0) {
    gst(q_idx + i, ok ? q : (int64_t)-1);
    gst(r_idx + i, ok ? r : (int64_t)-1);
  }
  const V* g = reinterpret_cast<const V*>(gu + i * (int64_t)dim);
  V* qo = reinterpret_cast<V*>(q_val + i * (int64_t)q_dim);
  V* ro = reinterpret_cast<V*>(r_val + i * (int64_t)r_dim);
  const V* qrow = reinterpret_cast<const V*>(qt + qc * (int64_t)q_dim);
  const V* rrow = reinterpret_cast<const V*>(rt + rc * (int64_t)r_dim);
  for (int c = col0; c < W; c += lanes) {
    const V gv = ok ? gld(g + c) : vzero<V>();
    if (cat) {
      if (c < dvq)
        gst(qo + c, gv);
      else
        gst(ro + (c - dvq), gv);
    } else if (op == DR_MHV_MUL) {
      // one fp32 multiply per element; the factor rows as they stand
      const V a = gld(qrow + c), b = gld(rrow + c);
      gst(qo + c, ok ? vmulv(gv, b) : vzero<V>());
      gst(ro + c, ok ? vmulv(gv, a) : vzero<V>());
    } else {
      gst(qo + c, gv);
      if (ro != qo) gst(ro + c, gv);
    }
  }
}

static int check_pair(const float* q_table, int64_t q_rows, int q_dim, const float* r_table,
                      int64_t r_rows, int r_dim, int operation) {
  DR_REQUIRE(q_table && r_table, DR_INVALID_ARGUMENT, "multihash: null table");
  DR_REQUIRE(q_rows >= 1 && r_rows >= 1 && q_dim >= 1 && r_dim >= 1, DR_INVALID_ARGUMENT,
             "multihash: rows and dims must be >= 1");
  DR_REQUIRE(operation == DR_MHV_ADD || operation == DR_MHV_MUL || operation == DR_MHV_CONCAT,
             DR_INVALID_ARGUMENT, "multihash: unknown operation %d", operation);
  DR_REQUIRE(operation == DR_MHV_CONCAT || q_dim == r_dim, DR_INVALID_ARGUMENT,
             "multihash: add / mul need q_dim == r_dim (%d vs %d)", q_dim, r_dim);
  return DR_OK;
}

}  // namespace dr

extern "C" {

int dr_mhv_lookup_sparse_grouped(const dr_mhv_desc* descs_host, int num_tables, int64_t batch,
                                 void* stream) {
  return dr::run_mhv(descs_host, num_tables, batch, nullptr, dr::S(stream));
}

int dr_mhv_gather(const float* q_table, int64_t q_rows, int q_dim, const float* r_table,
                  int64_t r_rows, int r_dim, int operation, const int64_t* ids, int64_t n,
                  const int64_t* n_dev, float* out, void* stream) {
  using namespace dr;
  int rc = check_pair(q_table, q_rows, q_dim, r_table, r_rows, r_dim, operation);
  if (rc) return rc;
  DR_REQUIRE(n >= 0, DR_INVALID_ARGUMENT, "multihash gather: negative n");
  DR_REQUIRE(ids && out, DR_INVALID_ARGUMENT, "multihash gather: null ids or out");
  // the one-hot pooled lookup of n bags of one id, into [n, dim] rows
  dr_mhv_desc d;
  memset(&d, 0, sizeof(d));
  d.q_table = q_table;
  d.q_rows = q_rows;
  d.q_dim = q_dim;
  d.r_table = r_table;
  d.r_rows = r_rows;
  d.r_dim = r_dim;
  d.operation = operation;
  d.combiner = DR_COMBINER_SUM;
  d.ids = ids;
  d.out = out;
  d.out_stride = operation == DR_MHV_CONCAT ? (int64_t)q_dim + r_dim : (int64_t)q_dim;
  return run_mhv(&d, 1, n, n_dev, S(stream));
}

int dr_mhv_grad(const float* q_table, int64_t q_rows, int q_dim, const float* r_table,
                int64_t r_rows, int r_dim, int operation, const int64_t* uniq, const float* gu,
                int64_t n, const int64_t* n_dev, int64_t* q_idx, int64_t* r_idx, float* q_val,
                float* r_val, void* stream) {
  using namespace dr;
  int rc = check_pair(q_table, q_rows, q_dim, r_table, r_rows, r_dim, operation);
  if (rc) return rc;
  DR_REQUIRE(n >= 0, DR_INVALID_ARGUMENT, "multihash grad: negative n");
  DR_REQUIRE(uniq && gu && q_idx && r_idx && q_val && r_val, DR_INVALID_ARGUMENT,
             "multihash grad: null pointer");
  DR_REQUIRE(q_val != r_val || operation == DR_MHV_ADD, DR_INVALID_ARGUMENT,
             "multihash grad: q_val and r_val may coincide for DR_MHV_ADD only");
  DR_REQUIRE(q_idx != r_idx, DR_INVALID_ARGUMENT, "multihash grad: q_idx and r_idx coincide");
  if (n == 0) return DR_OK;
  const bool v4 = q_dim % 4 == 0 && r_dim % 4 == 0 && aligned16(q_table) && aligned16(r_table) &&
                  aligned16(gu) && aligned16(q_val) && aligned16(r_val);
  const int vec = v4 ? 4 : 1;
  const int W = (operation == DR_MHV_CONCAT ? q_dim + r_dim : q_dim) / vec;
  int shift = 0;
  while (shift < 8 && (1 << shift) < W) ++shift;
  const unsigned blocks = (unsigned)ceil_div(n, 256 >> shift);
  hipStream_t s = S(stream);
  if (v4)
    hipLaunchKernelGGL(mhv_grad_kernel<4>, dim3(blocks), dim3(256), 0, s, q_table, q_rows, q_dim,
                       r_table, r_rows, r_dim, operation, uniq, gu, n, n_dev, q_idx, r_idx, q_val,
                       r_val, shift);
  else
    hipLaunchKernelGGL(mhv_grad_kernel<1>, dim3(blocks), dim3(256), 0, s, q_table, q_rows, q_dim,
                       r_table, r_rows, r_dim, operation, uniq, gu, n, n_dev, q_idx, r_idx, q_val,
                       r_val, shift);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

}  // extern "C"
