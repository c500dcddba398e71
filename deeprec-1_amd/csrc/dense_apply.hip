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
// dr_dense_apply_grouped_ex adds dense Adam, FTRL and AdagradDecay to the same
// three steps: FTRL's elementwise update and AdagradDecay's per-row int64
// count live in the apply kernel; dense Adam is non-lazy, so the apply kernel
// also sets one bit per named (table, row) in a workspace bitmap (cleared per
// launch group) and
//
//   sweep  streams every row whose bit is clear once: m, v decay, the row moves.
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

// One element of a named row.  OPT is dr_opt_elem.h's code; OPT_ADAM here is
// the dense (non-lazy) Adam, whose named rows take AdamAsync's element.
template <int OPT>
__device__ __forceinline__ float da_one(float g, float w, float* a1, float* a2,
                                        const OptScalars& sc, bool dec) {
  if (OPT == OPT_FTRL) return ftrl_dense_one(g, w, a1, a2, sc);
  if (OPT == OPT_ADAGRAD_DECAY) return adagrad_decay_one(g, w, a1, dec, sc);
  if (OPT == OPT_ADAM) return apply_one<OPT_ADAM_ASYNC, 1, 1>(g, w, a1, a2, sc);
  return apply_one<OPT, 1, 1>(g, w, a1, a2, sc);
}
template <int OPT>
__device__ __forceinline__ void da_elem(float4& w, const float4& g, float4& a1, float4& a2,
                                        const OptScalars& sc, bool dec) {
  w.x = da_one<OPT>(g.x, w.x, &a1.x, &a2.x, sc, dec);
  w.y = da_one<OPT>(g.y, w.y, &a1.y, &a2.y, sc, dec);
  w.z = da_one<OPT>(g.z, w.z, &a1.z, &a2.z, sc, dec);
  w.w = da_one<OPT>(g.w, w.w, &a1.w, &a2.w, sc, dec);
}
template <int OPT>
__device__ __forceinline__ void da_elem(float& w, const float& g, float& a1, float& a2,
                                        const OptScalars& sc, bool dec) {
  w = da_one<OPT>(g, w, &a1, &a2, sc, dec);
}

// What the optimizers of dr_dense_apply_grouped_ex add to a launch:
// AdagradDecay's global_step / decay_step, and dense Adam's bitmap of named
// rows (one bit per row; table t's words start at bits + boff[t]) with the
// sweep's element offsets (eoff[t]: first VEC-wide element of table t).
struct DaExtra {
  int64_t epoch;
  uint32_t* bits;
  int64_t boff[DR_MAX_GROUP];
  int64_t eoff[DR_MAX_GROUP + 1];
};
static_assert(sizeof(DaArgs) + sizeof(DaExtra) + sizeof(OptScalars) + 64 <= 4096,
              "dense apply kernel arguments exceed 4 KiB");

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
                                                       OptScalars sc, DaExtra ex) {
  using V = typename VecT<VEC>::T;
  __shared__ DaTable sd[DR_MAX_GROUP];  // per-lane table index: stage in LDS
  __shared__ int64_t soff[DR_MAX_GROUP + 1];
  __shared__ int heads[256];
  __shared__ int nheads;
  __shared__ int64_t sboff[OPT == OPT_ADAM ? DR_MAX_GROUP : 1];
  if (threadIdx.x < T) sd[threadIdx.x] = a.t[threadIdx.x];
  if (threadIdx.x <= T) soff[threadIdx.x] = a.off[threadIdx.x];
  if (OPT == OPT_ADAM && threadIdx.x < T) sboff[threadIdx.x] = ex.boff[threadIdx.x];
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
  // slot2 as a third row column (AdagradDecay's is the int64 [rows] count)
  constexpr bool S2 = OPT == OPT_ADAM_ASYNC || OPT == OPT_ADAM_RMSPROP || OPT == OPT_ADAM ||
                      OPT == OPT_FTRL;
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
    if (OPT == OPT_ADAM_ASYNC || OPT == OPT_ADAM) {
      // alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power) in float, from the
      // powers as they stand (ev_apply_kernel's expression); da_powers_kernel
      // advances AdamAsync's after this launch, dense Adam's are the caller's
      const float b1p = gld(d.powers), b2p = gld(d.powers + 1);
      sh.alpha = sh.lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
    }
    bool dec = false;
    if (OPT == OPT_ADAGRAD_DECAY) {
      // one count per row: the row decays when the step's epoch is past it; the
      // run's first lane writes it back (every lane of the group read the old one)
      int64_t* cnt = reinterpret_cast<int64_t*>(d.s2) + row;
      const int64_t seen = gld(cnt);
      dec = ex.epoch > seen;
      if (dec && lg == 0) gst(cnt, seen + 1);
    }
    if (OPT == OPT_ADAM && lg == 0)   // the sweep leaves this row alone
      atomicOr(ex.bits + sboff[t] + (row >> 5), 1u << (row & 31));
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int col = lg + c * G;
      if (col >= dv) continue;
      da_elem<OPT>(w[c], acc.v[c], a1[c], a2[c], sh, dec);
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

// Dense Adam, the rows no gradient named (bit clear in the bitmap the apply
// kernel filled; all of them when the group has no positions): every row of
// every table of the group is read and written once, by this sweep or by the
// run that owns it.  The group's tables are one flat range of VEC-wide
// elements (4-wide shapes: dim % 4 == 0, so an element never straddles rows);
// a thread takes kDaSweepPer of them a block-width apart, loads first and
// unconditionally (past the end: the last element again), stores under the
// select.
static constexpr int kDaSweepPer = 4;

__device__ __forceinline__ void da_unnamed(float4& w, float4& m, float4& v, const OptScalars& sc) {
  w.x = adam_unnamed_one(w.x, &m.x, &v.x, sc);
  w.y = adam_unnamed_one(w.y, &m.y, &v.y, sc);
  w.z = adam_unnamed_one(w.z, &m.z, &v.z, sc);
  w.w = adam_unnamed_one(w.w, &m.w, &v.w, sc);
}
__device__ __forceinline__ void da_unnamed(float& w, float& m, float& v, const OptScalars& sc) {
  w = adam_unnamed_one(w, &m, &v, sc);
}

template <int VEC>
__global__ __launch_bounds__(256) void da_adam_sweep_kernel(DaArgs a, int T, OptScalars sc,
                                                            DaExtra ex) {
  using V = typename VecT<VEC>::T;
  __shared__ DaTable sd[DR_MAX_GROUP];  // per-lane table index: stage in LDS
  __shared__ int64_t seoff[DR_MAX_GROUP + 1];
  __shared__ int64_t sboff[DR_MAX_GROUP];
  if (threadIdx.x < T) sd[threadIdx.x] = a.t[threadIdx.x];
  if (threadIdx.x < T) sboff[threadIdx.x] = ex.boff[threadIdx.x];
  if (threadIdx.x <= T) seoff[threadIdx.x] = ex.eoff[threadIdx.x];
  __syncthreads();
  const int64_t total = seoff[T];   // (>= 1: every table has rows >= 1, dim >= VEC)
  const int64_t first = (int64_t)blockIdx.x * (256 * kDaSweepPer);
  V *wp[kDaSweepPer], *mp[kDaSweepPer], *vp[kDaSweepPer];
  V w[kDaSweepPer], m[kDaSweepPer], v[kDaSweepPer];
  float b1p[kDaSweepPer], b2p[kDaSweepPer];
  uint32_t word[kDaSweepPer];
  int bit[kDaSweepPer];
  bool in[kDaSweepPer];
#pragma unroll
  for (int u = 0; u < kDaSweepPer; ++u) {
    const int64_t e = first + u * 256 + threadIdx.x;
    in[u] = e < total;
    const int64_t ec = in[u] ? e : total - 1;
    const int t = table_of(seoff, T, ec, first);
    const DaTable& d = sd[t];
    const int64_t k = ec - seoff[t];   // the table's k-th element, row k / (dim / VEC)
    const int dv = d.dim / VEC;
    const int64_t row = seoff[t + 1] - seoff[t] <= (int64_t)0xffffffffu
                            ? (int64_t)((uint32_t)k / (uint32_t)dv)
                            : k / dv;
    wp[u] = reinterpret_cast<V*>(d.table) + k;
    mp[u] = reinterpret_cast<V*>(d.s1) + k;
    vp[u] = reinterpret_cast<V*>(d.s2) + k;
    word[u] = gld(ex.bits + sboff[t] + (row >> 5));
    bit[u] = (int)(row & 31);
    b1p[u] = gld(d.powers);
    b2p[u] = gld(d.powers + 1);
    w[u] = gld(wp[u]);
    m[u] = gld(mp[u]);
    v[u] = gld(vp[u]);
  }
#pragma unroll
  for (int u = 0; u < kDaSweepPer; ++u) {
    OptScalars sh = sc;
    sh.alpha = sh.lr * sqrtf(1.0f - b2p[u]) / (1.0f - b1p[u]);   // the apply kernel's expression
    da_unnamed(w[u], m[u], v[u], sh);
    if (in[u] && !((word[u] >> bit[u]) & 1u)) {
      gst(mp[u], m[u]);
      gst(vp[u], v[u]);
      gst(wp[u], w[u]);
    }
  }
}

template <int OPT, int VEC, int G, int CPL>
static int launch_da(const DaArgs& a, int T, int rbits, const uint64_t* skeys,
                     const int32_t* svals, const OptScalars& sc, const DaExtra& ex,
                     hipStream_t s) {
  const int64_t total = a.off[T];
  hipLaunchKernelGGL((da_apply_kernel<OPT, VEC, G, CPL>),
                     dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, a, T, rbits,
                     skeys, svals, sc, ex);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

static bool da_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// (AdagradDecay's slot2 is the int64 [rows] count, not a row column)
static bool da_v4(const dr_dense_apply_desc& d, int optimizer) {
  return d.dim % 4 == 0 && da_aligned16(d.table) && da_aligned16(d.slot1) &&
         (optimizer == DR_OPT_ADAGRAD_DECAY || da_aligned16(d.slot2)) && da_aligned16(d.grad);
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
static int da_shape(const dr_dense_apply_desc& d, int optimizer) {
  if (d.dim < 1) return -1;
  if (da_v4(d, optimizer)) {
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
                       const int32_t* svals, const OptScalars& sc, const DaExtra& ex, int shape,
                       hipStream_t s) {
#define DR_DA(K, V, G, C) \
  case K:                 \
    return launch_da<OPT, V, G, C>(a, T, rbits, skeys, svals, sc, ex, s)
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
static DaPlan da_plan(const dr_dense_apply_desc* descs, int num_tables, int optimizer) {
  DaPlan p;
  p.order.resize(num_tables);
  std::vector<int> shape(num_tables);
  for (int t = 0; t < num_tables; ++t) p.order[t] = t, shape[t] = da_shape(descs[t], optimizer);
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
// Dense Adam adds `words` 32-bit words of named-row bits (after the rest, so
// the other optimizers' workspace is what it was).
static size_t da_group_ws(int64_t total, int64_t words) {
  if (total <= 0 && words <= 0) return 0;
  Carver c(nullptr);
  if (total > 0) {
    c.take<uint64_t>(total);
    c.take<uint64_t>(total);
    c.take<int32_t>(total);
    c.take<int32_t>(total);
    c.take<char>(dr_sort_pairs_workspace_size(total));
  }
  if (words > 0) c.take<uint32_t>(words);
  return c.used + 256;
}

static int64_t da_bit_words(int64_t rows) { return rows >= 1 ? (rows + 31) / 32 : 0; }

static size_t da_ws_bytes(int optimizer, const dr_dense_apply_desc* descs, int num_tables) {
  // the largest group's: the groups run one after another on the stream
  size_t need = 0;
  const DaPlan plan = da_plan(descs, num_tables, optimizer);
  for (int g = 0; g < plan.groups(); ++g) {
    int64_t total = 0, words = 0;
    for (int k = plan.start[g]; k < plan.start[g + 1]; ++k) {
      const dr_dense_apply_desc& d = descs[plan.order[k]];
      if (d.n > 0 && d.n < ((int64_t)1 << 31)) total += d.n;   // (others are refused by the entry)
      if (optimizer == DR_OPT_ADAM && bit_length((uint64_t)d.rows) <= 56)
        words += da_bit_words(d.rows);
    }
    need = std::max(need, da_group_ws(total, words));
  }
  return need;
}

// Everything that can be refused is refused here, before a device is touched.
// `ex`: the call came through dr_dense_apply_grouped_ex, which also takes
// dense Adam, FTRL and AdagradDecay (lr and opts are theirs).
static int da_validate(int optimizer, bool ex, const dr_dense_apply_desc* descs, int num_tables,
                       float lr, const dr_dense_apply_opts* opts, const void* ws,
                       size_t ws_bytes) {
  const bool base = optimizer == DR_OPT_SGD || optimizer == DR_OPT_ADAGRAD ||
                    optimizer == DR_OPT_ADAM_ASYNC || optimizer == DR_OPT_ADAM_ASYNC_RMSPROP;
  if (!ex)
    DR_REQUIRE(base, DR_INVALID_ARGUMENT,
               "dense apply: optimizer %d is not SGD, Adagrad or AdamAsync[+RMSprop]", optimizer);
  DR_REQUIRE(base || optimizer == DR_OPT_ADAM || optimizer == DR_OPT_FTRL ||
                 optimizer == DR_OPT_ADAGRAD_DECAY,
             DR_INVALID_ARGUMENT, "dense apply: unknown optimizer %d", optimizer);
  if (optimizer == DR_OPT_FTRL || optimizer == DR_OPT_ADAGRAD_DECAY)
    DR_REQUIRE(opts, DR_INVALID_ARGUMENT, "dense apply: optimizer %d needs opts", optimizer);
  if (optimizer == DR_OPT_FTRL)
    DR_REQUIRE(lr != 0.0f, DR_INVALID_ARGUMENT, "dense apply: FTRL divides by lr, which is 0");
  if (optimizer == DR_OPT_ADAGRAD_DECAY)
    DR_REQUIRE(opts->decay_step > 0, DR_INVALID_ARGUMENT,
               "dense apply: AdagradDecay needs decay_step > 0");
  DR_REQUIRE(num_tables >= 0, DR_INVALID_ARGUMENT, "dense apply: negative num_tables");
  DR_REQUIRE(descs || num_tables == 0, DR_INVALID_ARGUMENT, "dense apply: null descriptors");
  const bool s1 = optimizer != DR_OPT_SGD;
  const bool s2 = optimizer != DR_OPT_SGD && optimizer != DR_OPT_ADAGRAD;
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
    DR_REQUIRE((optimizer != DR_OPT_ADAM_ASYNC && optimizer != DR_OPT_ADAM) || d.powers,
               DR_INVALID_ARGUMENT,
               "dense apply table %d: Adam[Async] needs the device beta powers", t);
    DR_REQUIRE(optimizer != DR_OPT_ADAGRAD_DECAY || ((uintptr_t)d.slot2 & 7) == 0,
               DR_INVALID_ARGUMENT,
               "dense apply table %d: slot2 (the int64 decay count) is not 8-byte aligned", t);
    DR_REQUIRE(da_shape(d, optimizer) >= 0, DR_INVALID_ARGUMENT,
               "dense apply table %d: row width %d unsupported (max 1024 when a multiple of 4 "
               "and 16-byte aligned, else 256)", t, d.dim);
    DR_REQUIRE(bit_length((uint64_t)d.rows) <= (optimizer == DR_OPT_ADAM ? 40 : 56),
               DR_INVALID_ARGUMENT, "dense apply table %d: too many rows", t);
    for (int u = 0; u < t; ++u)
      DR_REQUIRE(descs[u].table != d.table, DR_INVALID_ARGUMENT,
                 "dense apply: descriptors %d and %d name the same table", u, t);
  }
  const DaPlan plan = da_plan(descs, num_tables, optimizer);
  for (int g = 0; g < plan.groups(); ++g) {
    int64_t total = 0;   // (every n < 2^31, at most DR_MAX_GROUP of them: no overflow)
    int64_t elems = 0;   // the Adam sweep's (rows <= 2^40 there, dim <= 1024: no overflow)
    for (int k = plan.start[g]; k < plan.start[g + 1]; ++k) {
      const dr_dense_apply_desc& d = descs[plan.order[k]];
      total += d.n;
      if (optimizer == DR_OPT_ADAM) elems += d.rows * d.dim;
    }
    DR_REQUIRE(total < ((int64_t)1 << 31), DR_INVALID_ARGUMENT,
               "dense apply: a launch group (up to %d tables of one row shape) holds >= 2^31 "
               "positions", DR_MAX_GROUP);
    DR_REQUIRE(elems < ((int64_t)1 << 40), DR_INVALID_ARGUMENT,
               "dense apply: a launch group's tables hold >= 2^40 elements (the Adam sweep's "
               "grid)");
  }
  const size_t need = da_ws_bytes(optimizer, descs, num_tables);
  DR_REQUIRE(need == 0 || (ws && ws_bytes >= need), DR_INVALID_ARGUMENT,
             "dense apply: workspace too small (%zu < %zu bytes)", ws ? ws_bytes : (size_t)0, need);
  return DR_OK;
}

static int da_run(int optimizer, bool is_ex, const dr_dense_apply_desc* descs, int num_tables,
                  float lr, float beta1, float beta2, float epsilon,
                  const dr_dense_apply_opts* opts, void* ws, size_t ws_bytes, hipStream_t s) {
  int rc = da_validate(optimizer, is_ex, descs, num_tables, lr, opts, ws, ws_bytes);
  if (rc) return rc;
  OptScalars sc{};
  sc.lr = lr;
  sc.beta1 = beta1;
  sc.beta2 = beta2;
  sc.eps = epsilon;
  int64_t epoch = 0;
  if (optimizer == DR_OPT_FTRL) {
    sc.l1 = opts->l1;
    sc.l2 = opts->l2;
    sc.lr_power = opts->lr_power;
    sc.l2_shrinkage = opts->l2_shrinkage;
  } else if (optimizer == DR_OPT_ADAGRAD_DECAY) {
    sc.decay_rate = opts->decay_rate;
    sc.decay_baseline = opts->decay_baseline;
    sc.decay_step = opts->decay_step;
    epoch = opts->global_step / opts->decay_step;
  }
  const bool adam = optimizer == DR_OPT_ADAM;
  int* st = nullptr;
  const DaPlan plan = da_plan(descs, num_tables, optimizer);
  for (int g = 0; g < plan.groups(); ++g) {
    const int* members = plan.order.data() + plan.start[g];
    const int T = plan.start[g + 1] - plan.start[g];
    const int shape = da_shape(descs[members[0]], optimizer);   // the whole group's
    const int vec = shape <= 8 ? 4 : 1;
    DaArgs a;
    memset(&a, 0, sizeof(a));
    DaPowers pw;
    memset(&pw, 0, sizeof(pw));
    DaExtra ex;
    memset(&ex, 0, sizeof(ex));
    ex.epoch = epoch;
    int64_t words = 0;
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
      if (adam) {
        ex.boff[t] = words;
        words += da_bit_words(d.rows);
        ex.eoff[t + 1] = ex.eoff[t] + d.rows * (d.dim / vec);
      }
    }
    const int64_t total = a.off[T];
    // every count is 0: nothing changes, the powers included -- but a table
    // that is in a dense Adam call steps (its rows decay and move) all the same
    if (total == 0 && !adam) continue;
    Carver c(ws);
    uint64_t *keys = nullptr, *skeys = nullptr;
    int32_t *vals = nullptr, *svals = nullptr;
    void* sort_ws = nullptr;
    const size_t sort_bytes = total > 0 ? dr_sort_pairs_workspace_size(total) : 0;
    if (total > 0) {   // (da_group_ws's order)
      keys = c.take<uint64_t>(total);
      skeys = c.take<uint64_t>(total);
      vals = c.take<int32_t>(total);
      svals = c.take<int32_t>(total);
      sort_ws = c.take<char>(sort_bytes);
    }
    if (adam) {
      // the workspace is reused from group to group: the bits are cleared for
      // each (by a kernel: fill_bytes' reason)
      ex.bits = c.take<uint32_t>(words);
      rc = fill_bytes(ex.bits, 0, (size_t)words * sizeof(uint32_t), s);
      if (rc) return rc;
    }
    if (total > 0) {
      if (!st) {
        st = status_word();
        DR_REQUIRE(st, DR_INTERNAL, "status word unavailable");
      }
      // a row id is < rows <= 2^rbits - 1, so no live key is all ones
      const int rbits = bit_length((uint64_t)max_rows);
      const int bits = rbits + bit_length((uint64_t)(T - 1));
      hipLaunchKernelGGL(da_keys_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, a,
                         T, rbits, keys, vals, st);
      DR_LAUNCH_CHECK();
      rc = dr_sort_pairs(keys, vals, skeys, svals, total, 0, bits, sort_ws, sort_bytes, s);
      if (rc) return rc;
      switch (optimizer) {
        case DR_OPT_SGD:
          rc = dispatch_da<OPT_SGD>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
        case DR_OPT_ADAGRAD:
          rc = dispatch_da<OPT_ADAGRAD>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
        case DR_OPT_ADAM_ASYNC:
          rc = dispatch_da<OPT_ADAM_ASYNC>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
        case DR_OPT_ADAM_ASYNC_RMSPROP:
          rc = dispatch_da<OPT_ADAM_RMSPROP>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
        case DR_OPT_ADAM:
          rc = dispatch_da<OPT_ADAM>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
        case DR_OPT_FTRL:
          rc = dispatch_da<OPT_FTRL>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
        default:
          rc = dispatch_da<OPT_ADAGRAD_DECAY>(a, T, rbits, skeys, svals, sc, ex, shape, s);
          break;
      }
      if (rc) return rc;
      if (optimizer == DR_OPT_ADAM_ASYNC) {
        hipLaunchKernelGGL(da_powers_kernel, dim3(1), dim3(64), 0, s, pw, T, beta1, beta2);
        DR_LAUNCH_CHECK();
      }
    }
    if (adam) {
      const unsigned blocks = (unsigned)ceil_div(ex.eoff[T], 256 * kDaSweepPer);
      if (vec == 4)
        hipLaunchKernelGGL(da_adam_sweep_kernel<4>, dim3(blocks), dim3(256), 0, s, a, T, sc, ex);
      else
        hipLaunchKernelGGL(da_adam_sweep_kernel<1>, dim3(blocks), dim3(256), 0, s, a, T, sc, ex);
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
  return dr::da_ws_bytes(DR_OPT_SGD, descs_host, num_tables);
}

int dr_dense_apply_grouped(int optimizer, const dr_dense_apply_desc* descs_host, int num_tables,
                           float lr, float beta1, float beta2, float epsilon, void* ws,
                           size_t ws_bytes, void* stream) {
  return dr::da_run(optimizer, false, descs_host, num_tables, lr, beta1, beta2, epsilon, nullptr,
                    ws, ws_bytes, dr::S(stream));
}

size_t dr_dense_apply_grouped_ex_workspace_size(int optimizer,
                                                const dr_dense_apply_desc* descs_host,
                                                int num_tables) {
  if (!descs_host || num_tables <= 0) return 0;
  return dr::da_ws_bytes(optimizer, descs_host, num_tables);
}

int dr_dense_apply_grouped_ex(int optimizer, const dr_dense_apply_desc* descs_host,
                              int num_tables, float lr, float beta1, float beta2, float epsilon,
                              const dr_dense_apply_opts* opts, void* ws, size_t ws_bytes,
                              void* stream) {
  return dr::da_run(optimizer, true, descs_host, num_tables, lr, beta1, beta2, epsilon, opts, ws,
                    ws_bytes, dr::S(stream));
}

}  // extern "C"
