// adaptive.hip -- AdaptiveEmbeddingVariable: the kernels between Unique, the
// EV resolve and the pooling.  An id's mask says whether it lives in the EV
// (a private row) or in the shared hash-bucket table; both are functions of
// the id, decided by the id's first position.
//
//   dr_adaptive_split  per-unique mask and bucket row, the stable compaction
//                      of the EV ids and their per-key default rows (the hash
//                      rows they have been training)
//   dr_adaptive_merge  the row selection of every unique id for the existing
//                      pooling (pool.hip select_row: >= 0 an EV pool row,
//                      -(h+1) row h of the hash table as the default block)
//   dr_adaptive_grad   the per-unique gradient split into the EV's compacted
//                      value block and the hash table's index vector
//
// The hash table is small and re-used: its rows are read with the default
// cache policy; the defaults block and the EV value block are written once
// and read once by the next kernel: nontemporal stores.  Row layout (VEC / G /
// CPL) and the row helpers are dr_rows.h's; row loads use always-valid
// pointers (indices clamped, load_row_u's reason).
#include "dr_adaptive.h"
#include "dr_common.h"
#include "dr_rows.h"

namespace dr {

__device__ __forceinline__ bool mask_at(const void* m, int bytes, int64_t k) {
  if (bytes == 1) return gld(static_cast<const uint8_t*>(m) + k) != 0;
  if (bytes == 4) return gld(static_cast<const int32_t*>(m) + k) != 0;
  return gld(static_cast<const int64_t*>(m) + k) != 0;
}

// first[u] = min{k : idx[k] == u}: an integer minimum, independent of the
// order the lanes run in (first starts as all ones, above every position).
__global__ __launch_bounds__(256) void adaptive_first_kernel(const int32_t* __restrict__ idx,
                                                             int64_t nnz, uint32_t* first) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnz) return;
  const uint32_t u = (uint32_t)gld(idx + k);
  if (u < (uint64_t)nnz) atomicMin(first + u, (uint32_t)k);
}

// Per unique id: the mask and the bucket row of its first position.  A
// supplied bucket row outside the table latches and becomes row 0.
__global__ __launch_bounds__(256) void adaptive_flags_kernel(
    const int64_t* __restrict__ uniq, const uint32_t* __restrict__ first, int64_t nnz,
    const int64_t* __restrict__ num_unique, const void* __restrict__ mask, int mask_bytes,
    const int64_t* __restrict__ hash, int64_t bucket_size, int32_t* __restrict__ mask_u,
    int64_t* __restrict__ hrow, int* st) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= eff_n(nnz, num_unique)) return;
  const uint32_t f = gld(first + u);
  int32_t m = 0;
  int64_t h = 0;
  if (f < (uint64_t)nnz) {
    m = mask_at(mask, mask_bytes, f) ? 1 : 0;
    h = hash ? gld(hash + f) : dr_adaptive_bucket(gld(uniq + u), bucket_size);
    if (!dr_adaptive_row_valid(h, bucket_size)) {
      latch(st, DR_INVALID_ARGUMENT);
      h = 0;
    }
  }
  gst(mask_u + u, m);
  gst(hrow + u, h);
}

// Stable compaction of the EV ids: unique u with mask_u[u] goes to position
// pre[u] (the exclusive scan of the flags), ascending in u.
__global__ __launch_bounds__(256) void adaptive_compact_kernel(
    const int64_t* __restrict__ uniq, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ mask_u, const int32_t* __restrict__ pre, int64_t n,
    const int64_t* __restrict__ num_unique, int64_t* __restrict__ ev_keys,
    int32_t* __restrict__ ev_src, int32_t* __restrict__ ev_counts) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= eff_n(n, num_unique) || !gld(mask_u + u)) return;
  const int64_t j = gld(pre + u);
  if ((uint64_t)j >= (uint64_t)n) return;
  gst(ev_keys + j, gld(uniq + u));
  gst(ev_src + j, (int32_t)u);
  if (ev_counts) gst(ev_counts + j, gld(counts + u));
}

// out[j] = table[sel ? sel[via[j]] : via[j]] for j < min(n, *n_dev), NB rows
// in flight per lane group.  via[j] is clamped into [0, n) and the selected
// row into [0, table_rows); rows past the count are neither read as rows nor
// written.  STREAM: the source rows are read once (nontemporal), else they are
// the re-used table (default policy).
template <int VEC, int G, int CPL, int NB, bool STREAM>
__global__ __launch_bounds__(256) void adaptive_rows_kernel(
    const float* __restrict__ table, int64_t table_rows, const int64_t* __restrict__ sel,
    const int32_t* __restrict__ via, int64_t n, const int64_t* __restrict__ n_dev,
    float* __restrict__ out, int dim) {
  constexpr int GPB = 256 / G;
  const int64_t j0 = ((int64_t)blockIdx.x * GPB + threadIdx.x / G) * NB;
  const int64_t ne = eff_n(n, n_dev);
  if (j0 >= ne) return;
  const int lg = threadIdx.x % G;
  const int dv = dim / VEC;
  Row<VEC, G, CPL> x[NB];
  bool live[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int64_t j = j0 + b;
    live[b] = j < ne;
    int64_t r = 0;
    if (live[b]) {
      int64_t u = gld(via + j);
      u = (uint64_t)u < (uint64_t)n ? u : 0;
      r = sel ? gld(sel + u) : u;
      r = (uint64_t)r < (uint64_t)table_rows ? r : 0;
    }
    const float* p = table + r * (int64_t)dim;
    if constexpr (STREAM)
      load_row_nt<VEC, G, CPL>(x[b], p, lg, dv);
    else
      load_row_u<VEC, G, CPL>(x[b], p, lg, dv);
  }
  wait_loads();
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (live[b]) store_row_nt<VEC, G, CPL>(x[b], out + (j0 + b) * (int64_t)dim, lg, dv);
}

static constexpr int kAdaptiveNB = 4;  // rows in flight per lane group

template <int VEC, int G, int CPL>
static int launch_rows(const float* table, int64_t table_rows, const int64_t* sel,
                       const int32_t* via, int64_t n, const int64_t* n_dev, float* out, int dim,
                       bool stream_src, hipStream_t s) {
  const int64_t items = ceil_div(n, kAdaptiveNB);
  const dim3 grid((unsigned)ceil_div(items, 256 / G));
  if (stream_src)
    hipLaunchKernelGGL((adaptive_rows_kernel<VEC, G, CPL, kAdaptiveNB, true>), grid, dim3(256), 0,
                       s, table, table_rows, sel, via, n, n_dev, out, dim);
  else
    hipLaunchKernelGGL((adaptive_rows_kernel<VEC, G, CPL, kAdaptiveNB, false>), grid, dim3(256),
                       0, s, table, table_rows, sel, via, n, n_dev, out, dim);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

// The fp32 row shapes of dispatch_pool<DR_ORDER_ALI> (pool.hip).
static bool adaptive_dim_ok(int dim, bool v4) { return dim >= 1 && dim <= (v4 ? 1024 : 256); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int dispatch_rows(const float* table, int64_t table_rows, const int64_t* sel,
                         const int32_t* via, int64_t n, const int64_t* n_dev, float* out, int dim,
                         bool v4, bool stream_src, hipStream_t s) {
#define DR_AD(V, G, C) \
  return launch_rows<V, G, C>(table, table_rows, sel, via, n, n_dev, out, dim, stream_src, s)
  if (v4) {
    const int d4 = dim / 4;
    if (d4 <= 1) DR_AD(4, 1, 1);
    if (d4 <= 2) DR_AD(4, 2, 1);
    if (d4 <= 4) DR_AD(4, 4, 1);
    if (d4 <= 8) DR_AD(4, 8, 1);
    if (d4 <= 16) DR_AD(4, 16, 1);
    if (d4 <= 32) DR_AD(4, 32, 1);
    if (d4 <= 64) DR_AD(4, 64, 1);
    if (d4 <= 128) DR_AD(4, 64, 2);
    if (d4 <= 256) DR_AD(4, 64, 4);
  } else {
    if (dim <= 4) DR_AD(1, 4, 1);
    if (dim <= 8) DR_AD(1, 8, 1);
    if (dim <= 16) DR_AD(1, 16, 1);
    if (dim <= 32) DR_AD(1, 32, 1);
    if (dim <= 64) DR_AD(1, 64, 1);
    if (dim <= 256) DR_AD(1, 64, 4);
  }
#undef DR_AD
  set_error("adaptive: row width %d unsupported", dim);
  return DR_INVALID_ARGUMENT;
}

// rows_u[u]: the EV pool row of an EV id whose resolve gave one, else
// -(hrow[u] + 1).  Lane i serves unique i (when it is a hash id) and
// compacted key i (an EV id, each named once by ev_src): disjoint targets.
__global__ __launch_bounds__(256) void adaptive_merge_kernel(
    const int32_t* __restrict__ mask_u, const int64_t* __restrict__ hrow,
    const int32_t* __restrict__ ev_src, const int64_t* __restrict__ ev_rows, int64_t n,
    const int64_t* __restrict__ num_unique, const int64_t* __restrict__ num_ev,
    int64_t* __restrict__ rows_u) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t U = eff_n(n, num_unique);
  if (i >= U) return;
  if (!gld(mask_u + i)) gst(rows_u + i, -(gld(hrow + i) + 1));
  if (i < eff_n(U, num_ev)) {
    const int64_t u = gld(ev_src + i);
    if ((uint64_t)u < (uint64_t)U && gld(mask_u + u)) {
      const int64_t r = gld(ev_rows + i);
      gst(rows_u + u, r >= 0 ? r : -(gld(hrow + u) + 1));
    }
  }
}

// hash_idx[u] = hrow[u] for a hash id, -1 for an EV id and past the count.
__global__ __launch_bounds__(256) void adaptive_hash_idx_kernel(
    const int32_t* __restrict__ mask_u, const int64_t* __restrict__ hrow, int64_t n,
    const int64_t* __restrict__ num_unique, int64_t* __restrict__ hash_idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t h = -1;
  if (i < eff_n(n, num_unique) && !gld(mask_u + i)) h = gld(hrow + i);
  gst(hash_idx + i, h);
}

struct AdaptiveWs {
  uint32_t* first;
  int32_t* pre;
  void* scan_ws;
  size_t bytes;
};

static AdaptiveWs carve_adaptive(void* base, int64_t n) {
  const size_t nn = (size_t)(n > 0 ? n : 1);
  Carver c(base);
  AdaptiveWs w;
  w.first = c.take<uint32_t>(nn);
  w.pre = c.take<int32_t>(nn);
  w.scan_ws = c.take<char>(scan_ws_bytes((int64_t)nn));
  w.bytes = c.used + 256;
  return w;
}

}  // namespace dr

extern "C" {

size_t dr_adaptive_split_workspace_size(int64_t nnz) {
  return dr::carve_adaptive(nullptr, nnz).bytes;
}

int dr_adaptive_split(const int64_t* uniq, const int32_t* idx, int64_t nnz,
                      const int64_t* num_unique, const void* mask, int mask_bytes,
                      const int64_t* hash, int64_t bucket_size, const float* hash_table, int dim,
                      const int32_t* counts, int32_t* mask_u, int64_t* hrow, int64_t* ev_keys,
                      int32_t* ev_src, int32_t* ev_counts, int64_t* num_ev, float* defaults,
                      void* ws, size_t ws_bytes, void* stream) {
  using namespace dr;
  DR_REQUIRE(nnz >= 0 && nnz < (int64_t)0x7FFFFFFF, DR_INVALID_ARGUMENT,
             "adaptive split: nnz must be in [0, 2^31 - 1)");
  DR_REQUIRE(uniq && idx && num_unique && mask && hash_table, DR_INVALID_ARGUMENT,
             "adaptive split: null uniq, idx, num_unique, mask or hash_table");
  DR_REQUIRE(mask_u && hrow && ev_keys && ev_src && num_ev && defaults, DR_INVALID_ARGUMENT,
             "adaptive split: null output");
  DR_REQUIRE(mask_bytes == 1 || mask_bytes == 4 || mask_bytes == 8, DR_INVALID_ARGUMENT,
             "adaptive split: mask elements of %d bytes (uint8, int32 or int64)", mask_bytes);
  DR_REQUIRE(bucket_size >= 1, DR_INVALID_ARGUMENT, "adaptive split: bucket_size must be >= 1");
  DR_REQUIRE((counts != nullptr) == (ev_counts != nullptr), DR_INVALID_ARGUMENT,
             "adaptive split: counts and ev_counts go together");
  const bool v4 = dim % 4 == 0 && aligned16(hash_table) && aligned16(defaults);
  DR_REQUIRE(adaptive_dim_ok(dim, v4), DR_INVALID_ARGUMENT,
             "adaptive split: row width %d unsupported (max 1024 when a multiple of 4 and "
             "16-byte aligned, else 256)", dim);
  AdaptiveWs w = carve_adaptive(ws, nnz);
  DR_REQUIRE(ws && ws_bytes >= w.bytes, DR_INVALID_ARGUMENT,
             "adaptive split: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
  hipStream_t s = S(stream);
  if (nnz == 0) return fill_bytes(num_ev, 0, sizeof(int64_t), s);
  int* st = status_word();
  DR_REQUIRE(st, DR_INTERNAL, "status word unavailable");
  int rc = fill_bytes(w.first, 0xFF, (size_t)nnz * sizeof(uint32_t), s);
  if (rc) return rc;
  const dim3 grid((unsigned)ceil_div(nnz, 256));
  hipLaunchKernelGGL(adaptive_first_kernel, grid, dim3(256), 0, s, idx, nnz, w.first);
  hipLaunchKernelGGL(adaptive_flags_kernel, grid, dim3(256), 0, s, uniq, w.first, nnz, num_unique,
                     mask, mask_bytes, hash, bucket_size, mask_u, hrow, st);
  DR_LAUNCH_CHECK();
  rc = scan_exclusive_i32(mask_u, w.pre, nnz, num_unique, num_ev, w.scan_ws, s);
  if (rc) return rc;
  hipLaunchKernelGGL(adaptive_compact_kernel, grid, dim3(256), 0, s, uniq, counts, mask_u, w.pre,
                     nnz, num_unique, ev_keys, ev_src, ev_counts);
  DR_LAUNCH_CHECK();
  // defaults[j] = hash_table[hrow[ev_src[j]]], j < Ue
  return dispatch_rows(hash_table, bucket_size, hrow, ev_src, nnz, num_ev, defaults, dim, v4,
                       false, s);
}

int dr_adaptive_merge(const int32_t* mask_u, const int64_t* hrow, const int32_t* ev_src,
                      const int64_t* ev_rows, int64_t n, const int64_t* num_unique,
                      const int64_t* num_ev, int64_t* rows_u, void* stream) {
  using namespace dr;
  DR_REQUIRE(n >= 0 && n < (int64_t)0x7FFFFFFF, DR_INVALID_ARGUMENT,
             "adaptive merge: n must be in [0, 2^31 - 1)");
  DR_REQUIRE(mask_u && hrow && ev_src && ev_rows && num_unique && num_ev && rows_u,
             DR_INVALID_ARGUMENT, "adaptive merge: null pointer");
  if (n == 0) return DR_OK;
  hipLaunchKernelGGL(adaptive_merge_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                     S(stream), mask_u, hrow, ev_src, ev_rows, n, num_unique, num_ev, rows_u);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

int dr_adaptive_grad(const float* gu, int dim, const int32_t* mask_u, const int64_t* hrow,
                     const int32_t* ev_src, int64_t n, const int64_t* num_unique,
                     const int64_t* num_ev, float* ev_val, int64_t* hash_idx, void* stream) {
  using namespace dr;
  DR_REQUIRE(n >= 0 && n < (int64_t)0x7FFFFFFF, DR_INVALID_ARGUMENT,
             "adaptive grad: n must be in [0, 2^31 - 1)");
  DR_REQUIRE(gu && mask_u && hrow && ev_src && num_unique && num_ev && ev_val && hash_idx,
             DR_INVALID_ARGUMENT, "adaptive grad: null pointer");
  DR_REQUIRE(gu != ev_val, DR_INVALID_ARGUMENT, "adaptive grad: ev_val must not be gu itself");
  const bool v4 = dim % 4 == 0 && aligned16(gu) && aligned16(ev_val);
  DR_REQUIRE(adaptive_dim_ok(dim, v4), DR_INVALID_ARGUMENT,
             "adaptive grad: row width %d unsupported (max 1024 when a multiple of 4 and "
             "16-byte aligned, else 256)", dim);
  if (n == 0) return DR_OK;
  hipStream_t s = S(stream);
  hipLaunchKernelGGL(adaptive_hash_idx_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s,
                     mask_u, hrow, n, num_unique, hash_idx);
  DR_LAUNCH_CHECK();
  // ev_val[j] = gu[ev_src[j]], j < Ue (each gradient row read once)
  return dispatch_rows(gu, n, nullptr, ev_src, n, num_ev, ev_val, dim, v4, true, s);
}

}  // extern "C"
