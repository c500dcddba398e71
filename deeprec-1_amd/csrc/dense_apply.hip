// dense_apply.hip -- grouped sparse apply for dense tables (the hash-bucket
// columns' tables and both halves of a MultiHashVariable): the optimizer's
// _deduplicate_indexed_slices (unique + unsorted_segment_sum) and the row
// update of ResourceSparseApply{GradientDescent,Adagrad,AdamAsync} in three
// steps on the device, with the gradient's row count read there.
//
//   keys   one (table slot, row) sort key per index position, value = the
//          position; positions past the device count, negative indices and
//          indices >= rows get the all-ones key (the last latches
//          DR_INVALID_ARGUMENT);
//   sort   the stable radix sort (scan_sort.hip) over the populated bits:
//          the positions of a (table, row) run come out ascending;
//   apply  a block finds the run heads among its 256 sorted positions; a
//          lane group per head walks the run, gsum = 0.0f + g[i0] + g[i1] +
//          ... as ONE serial fp32 chain per column (UnsortedSegmentSum
//          order, no float atomics), then updates and writes the row of the
//          table and of its slots once.
//
// Element math is dr_opt_elem.h's (the EV kernels' functions).  Gradient rows
// are read once (nontemporal); table and slot rows are the re-used data and
// take the default cache policy.  Loads are unconditional behind always-valid
// pointers, the selects come after them (load_row_u's reason).
#include <algorithm>
#include <vector>

#include "dr_common.h"
#include "dr_opt_elem.h"
#include "dr_rows.h"

namespace dr {

struct DaTable {
  float* table;
  float* s1;
  float* s2;
  const float* powers;
  const float* grad;
  const int64_t* idx;
  const int64_t* n_dev;
  int64_t n, rows;
  int32_t dim, pad;
};
struct DaArgs {
  DaTable t[DR_MAX_GROUP];
  int64_t off[DR_MAX_GROUP + 1];  // first global position of table t; off[T] = total
};
static_assert(sizeof(DaArgs) + 128 <= 4096, "dense apply kernel arguments exceed 4 KiB");

static constexpr uint64_t kDaNoKey = ~(uint64_t)0;

__global__ __launch_bounds__(256) void da_keys_kernel(DaArgs a, int T, int rbits,
                                                      uint64_t* __restrict__ keys,
                                                      int32_t* __restrict__ vals, int* st) {
  __shared__ DaTable sd[DR_MAX_GROUP];  // per-lane table index: stage in LDS
  __shared__ int64_t soff[DR_MAX_GROUP + 1];
  if (threadIdx.x < T) sd[threadIdx.x] = a.t[threadIdx.x];
  if (threadIdx.x <= T) soff[threadIdx.x] = a.off[threadIdx.x];
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * 256;
  const int64_t p = first + threadIdx.x;
  if (p >= soff[T]) return;
  const int t = table_of(soff, T, p, first);
  const DaTable& d = sd[t];
  const int64_t i = p - soff[t];
  // nothing at or past the count is read: entries there may hold anything
  const bool in = i < eff_n(d.n, d.n_dev);
  const int64_t r = in ? gld(d.idx + i) : (int64_t)-1;
  if (r >= d.rows) latch(st, DR_INVALID_ARGUMENT);  // skipped, as dr_gather does
  const bool ok = r >= 0 && r < d.rows;
  gst(keys + p, ok ? (((uint64_t)t << rbits) | (uint64_t)r) : kDaNoKey);
  gst(vals + p, (int32_t)p);
}

// A gradient row with the nontemporal policy, every load unconditional: a
// lane past the row's width reads column 0 again (dv >= 1) and its sum is
// never stored.
template <int VEC, int G, int CPL>
__device__ __forceinline__ void load_row_nt_u(Row<VEC, G, CPL>& x, const float* p, int lg, int dv) {
  using V = typename VecT<VEC>::T;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int col = lg + c * G;
    x.v[c] = nt_load(reinterpret_cast<const V*>(p) + (col < dv ? col : 0));
  }
}

// Per-component select (a ?: on the float4 struct goes through scratch).
__device__ __forceinline__ float4 da_sel(bool c, float4 a, float4 b) {
  return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
__device__ __forceinline__ float da_sel(bool c, float a, float b) { return c ? a : b; }

template <int OPT>
__device__ __forceinline__ void da_elem(float4& w, const float4& g, float4& a1, float4& a2,
                                        const OptScalars& sc) {
  w.x = apply_one<OPT, 4, 1>(g.x, w.x, &a1.x, &a2.x, sc);
  w.y = apply_one<OPT, 4, 1>(g.y, w.y, &a1.y, &a2.y, sc);
  w.z = apply_one<OPT, 4, 1>(g.z, w.z, &a1.z, &a2.z, sc);
  w.w = apply_one<OPT, 4, 1>(g.w, w.w, &a1.w, &a2.w, sc);
}
template <int OPT>
__device__ __forceinline__ void da_elem(float& w, const float& g, float& a1, float& a2,
                                        const OptScalars& sc) {
  w = apply_one<OPT, 1, 1>(g, w, &a1, &a2, sc);
}

// A block covers 256 sorted positions.  One lane per position finds the run
// heads (a live key that differs from its predecessor's) and queues them in
// LDS; the block's 256 / G lane groups then take the queued heads in turn
// (CPL column chunks of VEC floats per lane; the tables of a launch share one
// row shape, a table narrower than the shape leaves its last lanes idle).  A
// lane group per
// position would leave most of them idle: at 65 536 positions over 3 536 rows
// one position in 18 is a head.  The order in which heads are queued varies
// from launch to launch; every row's result is its own, so the values do not.
//
// A head walks its run kDaAhead positions at a time: the keys and positions
// of the next batch are requested before the gradient rows of this one are
// added (one dependent round trip per batch, not two), the rows are loaded
// together (clamped to the last position / the table's first gradient row
// where the run has ended) and added in order under a select.  The table and
// slot rows are requested before the walk and arrive during it.
static constexpr int kDaAhead = 4;

template <int OPT, int VEC, int G, int CPL>
__global__ __launch_bounds__(256) void da_apply_kernel(DaArgs a, int T, int rbits,
                                                       const uint64_t* __restrict__ skeys,
                                                       const int32_t* __restrict__ svals,
                                                       OptScalars sc) {
  using V = typename VecT<VEC>::T;
  __shared__ DaTable sd[DR_MAX_GROUP];  // per-lane table index: stage in LDS
  __shared__ int64_t soff[DR_MAX_GROUP + 1];
  __shared__ int heads[256];
  __shared__ int nheads;
  if (threadIdx.x < T) sd[threadIdx.x] = a.t[threadIdx.x];
  if (threadIdx.x <= T) soff[threadIdx.x] = a.off[threadIdx.x];
  if (threadIdx.x == 0) nheads = 0;
  __syncthreads();
  const int64_t total = soff[T];
  const int64_t first = (int64_t)blockIdx.x * 256;
  {
    const int64_t p = first + threadIdx.x;
    const int64_t pc = p < total ? p : total - 1;  // (total >= 1: nothing is launched for 0)
    const uint64_t key = gld(skeys + pc);
    const uint64_t prev = gld(skeys + (pc > 0 ? pc - 1 : 0));
    if (p < total && key != kDaNoKey && (p == 0 || prev != key))
      heads[atomicAdd(&nheads, 1)] = (int)threadIdx.x;
  }
  __syncthreads();
  const int nh = nheads;
  const int lg = threadIdx.x % G;
  constexpr bool S1 = OPT != OPT_SGD;
  constexpr bool S2 = opt_three_cols(OPT);
  for (int h = threadIdx.x / G; h < nh; h += 256 / G) {
    const int64_t p = first + heads[h];
    const uint64_t key = gld(skeys + p);
    const int t = (int)(key >> rbits);
    const int64_t row = (int64_t)(key & (((uint64_t)1 << rbits) - 1));
    const DaTable& d = sd[t];
    const int64_t dim = d.dim;
    const int dv = d.dim / VEC;
    const int64_t off = soff[t];
    const float* __restrict__ grad = d.grad;

    V* wp = reinterpret_cast<V*>(d.table + row * dim);
    V* p1 = reinterpret_cast<V*>((S1 ? d.s1 : d.table) + row * dim);
    V* p2 = reinterpret_cast<V*>((S2 ? d.s2 : d.table) + row * dim);
    V w[CPL], a1[CPL], a2[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int col = lg + c * G;
      const int cc = col < dv ? col : 0;  // (dv >= 1: column 0 exists)
      w[c] = gld(wp + cc);
      a1[c] = S1 ? gld(p1 + cc) : vzero<V>();
      a2[c] = S2 ? gld(p2 + cc) : vzero<V>();
    }

    uint64_t k[kDaAhead];
    int64_t pos[kDaAhead];
#pragma unroll
    for (int u = 0; u < kDaAhead; ++u) {
      const int64_t jc = p + u < total ? p + u : total - 1;
      k[u] = gld(skeys + jc);
      pos[u] = gld(svals + jc);
    }
    Row<VEC, G, CPL> acc;
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc.v[c] = vzero<V>();  // the sum starts from 0.0f
    for (int64_t j = p;; j += kDaAhead) {
      Row<VEC, G, CPL> x[kDaAhead];
      bool in[kDaAhead];
      bool run = true;
#pragma unroll
      for (int u = 0; u < kDaAhead; ++u) {
        run = run && j + u < total && k[u] == key;
        in[u] = run;
        load_row_nt_u<VEC, G, CPL>(x[u], grad + (run ? pos[u] - off : (int64_t)0) * dim, lg, dv);
      }
#pragma unroll
      for (int u = 0; u < kDaAhead; ++u) {
        const int64_t jn = j + kDaAhead + u;
        const int64_t jc = jn < total ? jn : total - 1;
        k[u] = gld(skeys + jc);
        pos[u] = gld(svals + jc);
      }
#pragma unroll
      for (int u = 0; u < kDaAhead; ++u)
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          acc.v[c] = da_sel(in[u], vadd(acc.v[c], x[u].v[c]), acc.v[c]);
        }
      if (!in[kDaAhead - 1]) break;
    }

    OptScalars sh = sc;
    if (OPT == OPT_ADAM_ASYNC) {
      // alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power) in float, from the
      // powers as they stand (ev_apply_kernel's expression); da_powers_kernel
      // advances them after this launch
      const float b1p = gld(d.powers), b2p = gld(d.powers + 1);
      sh.alpha = sh.lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int col = lg + c * G;
      if (col >= dv) continue;
      da_elem<OPT>(w[c], acc.v[c], a1[c], a2[c], sh);
      if (S1) gst(p1 + col, a1[c]);
      if (S2) gst(p2 + col, a2[c]);
      gst(wp + col, w[c]);
    }
  }
}

// AdamAsync: beta powers advance once per apply whose effective count is > 0
// (the op's `if (N > 0)`), after the rows -- ev_adam_powers_kernel's rule.
struct DaPowers {
  float* p[DR_MAX_GROUP];
  int64_t n[DR_MAX_GROUP];
  const int64_t* n_dev[DR_MAX_GROUP];
};
__global__ void da_powers_kernel(DaPowers a, int T, float beta1, float beta2) {
  const int t = threadIdx.x;
  if (t >= T || !a.p[t]) return;
  if (eff_n(a.n[t], a.n_dev[t]) <= 0) return;
  a.p[t][0] = a.p[t][0] * beta1;
  a.p[t][1] = a.p[t][1] * beta2;
}

template <int OPT, int VEC, int G, int CPL>
static int launch_da(const DaArgs& a, int T, int rbits, const uint64_t* skeys,
                     const int32_t* svals, const OptScalars& sc, hipStream_t s) {
  const int64_t total = a.off[T];
  hipLaunchKernelGGL((da_apply_kernel<OPT, VEC, G, CPL>),
                     dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, a, T, rbits,
                     skeys, svals, sc);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

static bool da_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool da_v4(const dr_dense_apply_desc& d) {
  return d.dim % 4 == 0 && da_aligned16(d.table) && da_aligned16(d.slot1) &&
         da_aligned16(d.slot2) && da_aligned16(d.grad);
}
static int bit_length(uint64_t x) {
  int b = 0;
  while (x) ++b, x >>= 1;
  return b;
}

// The row shape of ONE table (the shapes of multihash.hip / pool.hip): 4-wide
// (0 .. 8) when dim % 4 == 0 and table, slots and grad are 16-byte aligned,
// else scalar (9 .. 14); -1: no shape for this width.  Tables are launched
// with the tables of their own shape only (da_plan), so the shape a table
// validates for is the shape it runs, whatever else the call holds.
static int da_shape(const dr_dense_apply_desc& d) {
  if (d.dim < 1) return -1;
  if (da_v4(d)) {
    const int d4 = d.dim / 4;
    static const int lim[9] = {1, 2, 4, 8, 16, 32, 64, 128, 256};
    for (int k = 0; k < 9; ++k)
      if (d4 <= lim[k]) return k;
    return -1;
  }
  static const int lim[6] = {4, 8, 16, 32, 64, 256};
  for (int k = 0; k < 6; ++k)
    if (d.dim <= lim[k]) return 9 + k;
  return -1;
}

template <int OPT>
static int dispatch_da(const DaArgs& a, int T, int rbits, const uint64_t* skeys,
                       const int32_t* svals, const OptScalars& sc, int shape, hipStream_t s) {
#define DR_DA(K, V, G, C) \
  case K:                 \
    return launch_da<OPT, V, G, C>(a, T, rbits, skeys, svals, sc, s)
  switch (shape) {
    DR_DA(0, 4, 1, 1);
    DR_DA(1, 4, 2, 1);
    DR_DA(2, 4, 4, 1);
    DR_DA(3, 4, 8, 1);
    DR_DA(4, 4, 16, 1);
    DR_DA(5, 4, 32, 1);
    DR_DA(6, 4, 64, 1);
    DR_DA(7, 4, 64, 2);
    DR_DA(8, 4, 64, 4);
    DR_DA(9, 1, 4, 1);
    DR_DA(10, 1, 8, 1);
    DR_DA(11, 1, 16, 1);
    DR_DA(12, 1, 32, 1);
    DR_DA(13, 1, 64, 1);
    DR_DA(14, 1, 64, 4);
  }
#undef DR_DA
  set_error("dense apply: no row shape %d", shape);
  return DR_INTERNAL;
}

// Launch groups: the descriptors in shape order (stable), cut where the shape
// changes and every DR_MAX_GROUP tables.  order[start[g] .. start[g + 1]) are
// the descriptor indices of group g.
struct DaPlan {
  std::vector<int> order, start;
  int groups() const { return (int)start.size() - 1; }
};
static DaPlan da_plan(const dr_dense_apply_desc* descs, int num_tables) {
  DaPlan p;
  p.order.resize(num_tables);
  std::vector<int> shape(num_tables);
  for (int t = 0; t < num_tables; ++t) p.order[t] = t, shape[t] = da_shape(descs[t]);
  std::stable_sort(p.order.begin(), p.order.end(),
                   [&](int x, int y) { return shape[x] < shape[y]; });
  for (int k = 0; k < num_tables; ++k)
    if (k == 0 || shape[p.order[k]] != shape[p.order[k - 1]] ||
        k - p.start.back() == DR_MAX_GROUP)
      p.start.push_back(k);
  p.start.push_back(num_tables);
  return p;
}

// Workspace of one launch group over `total` positions: the key / position
// pairs before and after the sort, and the sort's own.
static size_t da_group_ws(int64_t total) {
  if (total <= 0) return 0;
  Carver c(nullptr);
  c.take<uint64_t>(total);
  c.take<uint64_t>(total);
  c.take<int32_t>(total);
  c.take<int32_t>(total);
  c.take<char>(dr_sort_pairs_workspace_size(total));
  return c.used + 256;
}

static size_t da_ws_bytes(const dr_dense_apply_desc* descs, int num_tables) {
  // the largest group's: the groups run one after another on the stream
  size_t need = 0;
  const DaPlan plan = da_plan(descs, num_tables);
  for (int g = 0; g < plan.groups(); ++g) {
    int64_t total = 0;
    for (int k = plan.start[g]; k < plan.start[g + 1]; ++k) {
      const int64_t n = descs[plan.order[k]].n;
      if (n > 0 && n < ((int64_t)1 << 31)) total += n;   // (others are refused by the entry)
    }
    need = std::max(need, da_group_ws(total));
  }
  return need;
}

// Everything that can be refused is refused here, before a device is touched.
static int da_validate(int optimizer, const dr_dense_apply_desc* descs, int num_tables,
                       const void* ws, size_t ws_bytes) {
  DR_REQUIRE(optimizer == DR_OPT_SGD || optimizer == DR_OPT_ADAGRAD ||
                 optimizer == DR_OPT_ADAM_ASYNC || optimizer == DR_OPT_ADAM_ASYNC_RMSPROP,
             DR_INVALID_ARGUMENT,
             "dense apply: optimizer %d is not SGD, Adagrad or AdamAsync[+RMSprop]", optimizer);
  DR_REQUIRE(num_tables >= 0, DR_INVALID_ARGUMENT, "dense apply: negative num_tables");
  DR_REQUIRE(descs || num_tables == 0, DR_INVALID_ARGUMENT, "dense apply: null descriptors");
  const bool s1 = optimizer != DR_OPT_SGD;
  const bool s2 = optimizer == DR_OPT_ADAM_ASYNC || optimizer == DR_OPT_ADAM_ASYNC_RMSPROP;
  for (int t = 0; t < num_tables; ++t) {
    const dr_dense_apply_desc& d = descs[t];
    DR_REQUIRE(d.table, DR_INVALID_ARGUMENT, "dense apply table %d: null table", t);
    DR_REQUIRE(d.rows >= 1 && d.dim >= 1 && d.n >= 0, DR_INVALID_ARGUMENT,
               "dense apply table %d: rows and dim must be >= 1, n >= 0", t);
    DR_REQUIRE(d.n < ((int64_t)1 << 31), DR_INVALID_ARGUMENT,
               "dense apply table %d: n >= 2^31 positions", t);
    DR_REQUIRE(d.n == 0 || (d.grad && d.idx), DR_INVALID_ARGUMENT,
               "dense apply table %d: null grad or idx", t);
    DR_REQUIRE((!s1 || d.slot1) && (!s2 || d.slot2), DR_INVALID_ARGUMENT,
               "dense apply table %d: the optimizer's slot is null", t);
    DR_REQUIRE(optimizer != DR_OPT_ADAM_ASYNC || d.powers, DR_INVALID_ARGUMENT,
               "dense apply table %d: AdamAsync needs the device beta powers", t);
    DR_REQUIRE(da_shape(d) >= 0, DR_INVALID_ARGUMENT,
               "dense apply table %d: row width %d unsupported (max 1024 when a multiple of 4 "
               "and 16-byte aligned, else 256)", t, d.dim);
    DR_REQUIRE(bit_length((uint64_t)d.rows) <= 56, DR_INVALID_ARGUMENT,
               "dense apply table %d: too many rows", t);
    for (int u = 0; u < t; ++u)
      DR_REQUIRE(descs[u].table != d.table, DR_INVALID_ARGUMENT,
                 "dense apply: descriptors %d and %d name the same table", u, t);
  }
  const DaPlan plan = da_plan(descs, num_tables);
  for (int g = 0; g < plan.groups(); ++g) {
    int64_t total = 0;   // (every n < 2^31, at most DR_MAX_GROUP of them: no overflow)
    for (int k = plan.start[g]; k < plan.start[g + 1]; ++k) total += descs[plan.order[k]].n;
    DR_REQUIRE(total < ((int64_t)1 << 31), DR_INVALID_ARGUMENT,
               "dense apply: a launch group (up to %d tables of one row shape) holds >= 2^31 "
               "positions", DR_MAX_GROUP);
  }
  const size_t need = da_ws_bytes(descs, num_tables);
  DR_REQUIRE(need == 0 || (ws && ws_bytes >= need), DR_INVALID_ARGUMENT,
             "dense apply: workspace too small (%zu < %zu bytes)", ws ? ws_bytes : (size_t)0, need);
  return DR_OK;
}

static int da_run(int optimizer, const dr_dense_apply_desc* descs, int num_tables, float lr,
                  float beta1, float beta2, float epsilon, void* ws, size_t ws_bytes,
                  hipStream_t s) {
  int rc = da_validate(optimizer, descs, num_tables, ws, ws_bytes);
  if (rc) return rc;
  OptScalars sc{};
  sc.lr = lr;
  sc.beta1 = beta1;
  sc.beta2 = beta2;
  sc.eps = epsilon;
  int* st = nullptr;
  const DaPlan plan = da_plan(descs, num_tables);
  for (int g = 0; g < plan.groups(); ++g) {
    const int* members = plan.order.data() + plan.start[g];
    const int T = plan.start[g + 1] - plan.start[g];
    const int shape = da_shape(descs[members[0]]);   // the whole group's
    DaArgs a;
    memset(&a, 0, sizeof(a));
    DaPowers pw;
    memset(&pw, 0, sizeof(pw));
    int64_t max_rows = 1;
    for (int t = 0; t < T; ++t) {
      const dr_dense_apply_desc& d = descs[members[t]];
      DaTable& o = a.t[t];
      o.table = d.table;
      o.s1 = d.slot1;
      o.s2 = d.slot2;
      o.powers = d.powers;
      o.grad = d.grad;
      o.idx = d.idx;
      o.n_dev = d.n_dev;
      o.n = d.n;
      o.rows = d.rows;
      o.dim = d.dim;
      a.off[t + 1] = a.off[t] + d.n;
      max_rows = std::max(max_rows, d.rows);
      pw.p[t] = optimizer == DR_OPT_ADAM_ASYNC ? d.powers : nullptr;
      pw.n[t] = d.n;
      pw.n_dev[t] = d.n_dev;
    }
    const int64_t total = a.off[T];
    if (total == 0) continue;  // every count is 0: nothing changes, the powers included
    if (!st) {
      st = status_word();
      DR_REQUIRE(st, DR_INTERNAL, "status word unavailable");
    }
    // a row id is < rows <= 2^rbits - 1, so no live key is all ones
    const int rbits = bit_length((uint64_t)max_rows);
    const int bits = rbits + bit_length((uint64_t)(T - 1));
    Carver c(ws);
    uint64_t* keys = c.take<uint64_t>(total);
    uint64_t* skeys = c.take<uint64_t>(total);
    int32_t* vals = c.take<int32_t>(total);
    int32_t* svals = c.take<int32_t>(total);
    const size_t sort_bytes = dr_sort_pairs_workspace_size(total);
    void* sort_ws = c.take<char>(sort_bytes);
    hipLaunchKernelGGL(da_keys_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, a, T,
                       rbits, keys, vals, st);
    DR_LAUNCH_CHECK();
    rc = dr_sort_pairs(keys, vals, skeys, svals, total, 0, bits, sort_ws, sort_bytes, s);
    if (rc) return rc;
    switch (optimizer) {
      case DR_OPT_SGD:
        rc = dispatch_da<OPT_SGD>(a, T, rbits, skeys, svals, sc, shape, s);
        break;
      case DR_OPT_ADAGRAD:
        rc = dispatch_da<OPT_ADAGRAD>(a, T, rbits, skeys, svals, sc, shape, s);
        break;
      case DR_OPT_ADAM_ASYNC:
        rc = dispatch_da<OPT_ADAM_ASYNC>(a, T, rbits, skeys, svals, sc, shape, s);
        break;
      default:
        rc = dispatch_da<OPT_ADAM_RMSPROP>(a, T, rbits, skeys, svals, sc, shape, s);
        break;
    }
    if (rc) return rc;
    if (optimizer == DR_OPT_ADAM_ASYNC) {
      hipLaunchKernelGGL(da_powers_kernel, dim3(1), dim3(64), 0, s, pw, T, beta1, beta2);
      DR_LAUNCH_CHECK();
    }
  }
  return DR_OK;
}

}  // namespace dr

extern "C" {

size_t dr_dense_apply_grouped_workspace_size(const dr_dense_apply_desc* descs_host,
                                             int num_tables) {
  if (!descs_host || num_tables <= 0) return 0;
  return dr::da_ws_bytes(descs_host, num_tables);
}

int dr_dense_apply_grouped(int optimizer, const dr_dense_apply_desc* descs_host, int num_tables,
                           float lr, float beta1, float beta2, float epsilon, void* ws,
                           size_t ws_bytes, void* stream) {
  return dr::da_run(optimizer, descs_host, num_tables, lr, beta1, beta2, epsilon, ws, ws_bytes,
                    dr::S(stream));
}

}  // extern "C"
