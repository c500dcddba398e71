// dense_ckpt.hip -- update marks and row export of dense tables: what a
// checkpoint or a delta of a DenseTable (a hash-bucket column's table, both
// tables of a MultiHashVariable, the hash table of an adaptive variable) and
// of its optimizer slots needs on the device.  The dense counterpart of the
// EV tracking kernels (ev_mark_updated_rows_kernel, ev_dirty_count_kernel).
//
//   mark     one lane per index position sets bit (row & 31) of word
//            (row >> 5); the bit is tested first, so a row marked again costs
//            a read and no atomic;
//   fill     every row marked (the last word's tail left 0), or none: kernels,
//            not memset nodes (dr_common.h, fill_bytes);
//   count    popcount of the valid bits;
//   export   popcount per word -> exclusive scan over the words -> the row ids
//            in ascending order -> a gather of the marked rows of up to
//            DR_DENSE_MAX_COLS columns (the table and its slots);
//   upsert   the gather's inverse: a delta's rows written over the table's.
//
// The bit arithmetic is dr_dense_bits.h's.  Row layout (VEC / G / CPL) and the
// row helpers are dr_rows.h's, the shapes those of dense_apply.hip; the row
// loads of a lane group are requested together behind always-valid pointers
// (indices clamped, load_row_u's reason), waited for once, then stored.
#include <algorithm>

#include "dr_common.h"
#include "dr_dense_bits.h"
#include "dr_rows.h"

namespace dr {

struct DcMarkTable {
  uint32_t* bits;
  const int64_t* idx;
  const int64_t* n_dev;
  int64_t n, rows;
};
struct DcMarkArgs {
  DcMarkTable t[DR_MAX_GROUP];
  int64_t off[DR_MAX_GROUP + 1];  // first global position of table t; off[T] = total
};
static_assert(sizeof(DcMarkArgs) + 128 <= 4096, "dense mark kernel arguments exceed 4 KiB");

__global__ __launch_bounds__(256) void dc_mark_kernel(DcMarkArgs a, int T) {
  __shared__ DcMarkTable sd[DR_MAX_GROUP];  // per-lane table index: stage in LDS
  __shared__ int64_t soff[DR_MAX_GROUP + 1];
  if (threadIdx.x < T) sd[threadIdx.x] = a.t[threadIdx.x];
  if (threadIdx.x <= T) soff[threadIdx.x] = a.off[threadIdx.x];
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * 256;
  const int64_t p = first + threadIdx.x;
  if (p >= soff[T]) return;
  const int t = table_of(soff, T, p, first);
  const DcMarkTable& d = sd[t];
  const int64_t i = p - soff[t];
  // nothing at or past the count is read: entries there may hold anything
  if (i < 0 || i >= eff_n(d.n, d.n_dev)) return;
  const int64_t row = gld(d.idx + i);
  if (row < 0 || row >= d.rows) return;  // skipped; the apply latches the error
  uint32_t* w = d.bits + dr_dense_bits_word(row);
  const uint32_t m = dr_dense_bits_mask(row);
  if (!(gld(w) & m)) atomicOr(w, m);
}

// bits[w] = all ? the valid bits of word w : 0.
__global__ __launch_bounds__(256) void dc_fill_kernel(uint32_t* __restrict__ bits, int64_t nw,
                                                      int64_t rows, int all) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= nw) return;
  gst(bits + w, all ? dr_dense_bits_valid(w, rows) : 0u);
}

// *total += popcount of the valid bits (the caller zeroed it on the stream).
__global__ __launch_bounds__(256) void dc_count_kernel(const uint32_t* __restrict__ bits,
                                                       int64_t nw, int64_t rows,
                                                       unsigned long long* __restrict__ total) {
  unsigned long long c = 0;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw;
       w += (int64_t)gridDim.x * blockDim.x)
    c += (unsigned)__popc(gld(bits + w) & dr_dense_bits_valid(w, rows));
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if (lane_id() == 0 && c) atomicAdd(total, c);
}

// cnt[w] = popcount of the valid bits of word w (the scan's input).
__global__ __launch_bounds__(256) void dc_popc_kernel(const uint32_t* __restrict__ bits,
                                                      int64_t nw, int64_t rows,
                                                      int32_t* __restrict__ cnt) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= nw) return;
  gst(cnt + w, (int32_t)__popc(gld(bits + w) & dr_dense_bits_valid(w, rows)));
}

// rows_out[pre[w] + rank] = 32 w + bit for every valid set bit of word w whose
// place is below `capacity`: ascending inside a word, and pre[] ascends.
__global__ __launch_bounds__(256) void dc_row_ids_kernel(const uint32_t* __restrict__ bits,
                                                         int64_t nw, int64_t rows,
                                                         const int32_t* __restrict__ pre,
                                                         int64_t capacity,
                                                         int64_t* __restrict__ rows_out) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= nw) return;
  uint32_t word = gld(bits + w) & dr_dense_bits_valid(w, rows);
  if (!word) return;
  int64_t j = gld(pre + w);
  if (j < 0) return;
  while (word && j < capacity) {
    const int b = __ffs((int)word) - 1;
    gst(rows_out + j, w * 32 + b);
    word &= word - 1;
    ++j;
  }
}

struct DcCols {
  const float* src[DR_DENSE_MAX_COLS];
  float* dst[DR_DENSE_MAX_COLS];
};

// One column per blockIdx.y, NB rows in flight per lane group, positions
// j < min(n, *n_dev).
//   gather (!SCATTER): dst[j] = src[idx[j]], idx = the exported row ids; the
//     source rows take the default policy (a table), the block written once is
//     stored nontemporal;
//   SCATTER: dst[idx[i]] = src[i]; an index outside [0, table_rows) is skipped
//     and latches; the value rows are read once (nontemporal).
// An out-of-range index is clamped to row 0 for the load and its row is not
// stored; nothing past the count is read as an index.
template <int VEC, int G, int CPL, int NB, bool SCATTER>
__global__ __launch_bounds__(256) void dc_rows_kernel(DcCols a, int64_t table_rows, int dim,
                                                      const int64_t* __restrict__ idx, int64_t n,
                                                      const int64_t* __restrict__ n_dev, int* st) {
  constexpr int GPB = 256 / G;
  const int64_t j0 = ((int64_t)blockIdx.x * GPB + threadIdx.x / G) * NB;
  const int64_t ne = eff_n(n, n_dev);
  if (j0 >= ne) return;
  const float* __restrict__ src = a.src[blockIdx.y];
  float* __restrict__ dst = a.dst[blockIdx.y];
  const int lg = threadIdx.x % G;
  const int dv = dim / VEC;
  Row<VEC, G, CPL> x[NB];
  bool live[NB];
  int64_t row[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int64_t j = j0 + b;
    live[b] = j < ne;
    int64_t r = 0;
    if (live[b]) {
      r = gld(idx + j);
      if ((uint64_t)r >= (uint64_t)table_rows) {
        if (SCATTER && blockIdx.y == 0) latch(st, DR_INVALID_ARGUMENT);
        live[b] = false;
        r = 0;
      }
    }
    row[b] = r;
    if constexpr (SCATTER)
      load_row_nt<VEC, G, CPL>(x[b], src + (j < ne ? j : j0) * (int64_t)dim, lg, dv);
    else
      load_row_u<VEC, G, CPL>(x[b], src + r * (int64_t)dim, lg, dv);
  }
  wait_loads();
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (!live[b]) continue;
    if constexpr (SCATTER)
      store_row<VEC, G, CPL>(x[b], dst + row[b] * (int64_t)dim, lg, dv);
    else
      store_row_nt<VEC, G, CPL>(x[b], dst + (j0 + b) * (int64_t)dim, lg, dv);
  }
}

static constexpr int kDcNB = 4;  // rows in flight per lane group

template <int VEC, int G, int CPL>
static int launch_dc_rows(bool scatter, const DcCols& a, int num_cols, int64_t table_rows, int dim,
                          const int64_t* idx, int64_t n, const int64_t* n_dev, int* st,
                          hipStream_t s) {
  const int64_t items = ceil_div(n, kDcNB);
  const dim3 grid((unsigned)ceil_div(items, 256 / G), (unsigned)num_cols);
  if (scatter)
    hipLaunchKernelGGL((dc_rows_kernel<VEC, G, CPL, kDcNB, true>), grid, dim3(256), 0, s, a,
                       table_rows, dim, idx, n, n_dev, st);
  else
    hipLaunchKernelGGL((dc_rows_kernel<VEC, G, CPL, kDcNB, false>), grid, dim3(256), 0, s, a,
                       table_rows, dim, idx, n, n_dev, st);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

static bool dc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The row shapes dense_apply.hip dispatches: 4-wide up to 1024 columns when
// dim % 4 == 0 and every pointer is 16-byte aligned, else scalar up to 256.
static bool dc_v4(int dim, const DcCols& a, int num_cols) {
  if (dim % 4) return false;
  for (int c = 0; c < num_cols; ++c)
    if (!dc_aligned16(a.src[c]) || !dc_aligned16(a.dst[c])) return false;
  return true;
}
static bool dc_dim_ok(int dim, bool v4) { return dim >= 1 && dim <= (v4 ? 1024 : 256); }

static int dispatch_dc_rows(bool scatter, bool v4, const DcCols& a, int num_cols,
                            int64_t table_rows, int dim, const int64_t* idx, int64_t n,
                            const int64_t* n_dev, int* st, hipStream_t s) {
#define DR_DC(V, G, C) \
  return launch_dc_rows<V, G, C>(scatter, a, num_cols, table_rows, dim, idx, n, n_dev, st, s)
  if (v4) {
    const int d4 = dim / 4;
    if (d4 <= 1) DR_DC(4, 1, 1);
    if (d4 <= 2) DR_DC(4, 2, 1);
    if (d4 <= 4) DR_DC(4, 4, 1);
    if (d4 <= 8) DR_DC(4, 8, 1);
    if (d4 <= 16) DR_DC(4, 16, 1);
    if (d4 <= 32) DR_DC(4, 32, 1);
    if (d4 <= 64) DR_DC(4, 64, 1);
    if (d4 <= 128) DR_DC(4, 64, 2);
    if (d4 <= 256) DR_DC(4, 64, 4);
  } else {
    if (dim <= 4) DR_DC(1, 4, 1);
    if (dim <= 8) DR_DC(1, 8, 1);
    if (dim <= 16) DR_DC(1, 16, 1);
    if (dim <= 32) DR_DC(1, 32, 1);
    if (dim <= 64) DR_DC(1, 64, 1);
    if (dim <= 256) DR_DC(1, 64, 4);
  }
#undef DR_DC
  set_error("dense rows: row width %d unsupported", dim);
  return DR_INVALID_ARGUMENT;
}

struct DcExportWs {
  int32_t* cnt;
  int32_t* pre;
  void* scan_ws;
  size_t bytes;
};
static DcExportWs carve_export(void* base, int64_t rows) {
  const size_t nw = (size_t)std::max<int64_t>(dr_dense_bits_words(rows), 1);
  Carver c(base);
  DcExportWs w;
  w.cnt = c.take<int32_t>(nw);
  w.pre = c.take<int32_t>(nw);
  w.scan_ws = c.take<char>(scan_ws_bytes((int64_t)nw));
  w.bytes = c.used + 256;
  return w;
}

static constexpr int64_t kDcMaxN = (int64_t)1 << 31;

static int dc_fill(uint32_t* bits, int64_t rows, int all, hipStream_t s) {
  DR_REQUIRE(bits, DR_INVALID_ARGUMENT, "dense marks: null bits");
  DR_REQUIRE(rows >= 1, DR_INVALID_ARGUMENT, "dense marks: rows must be >= 1");
  const int64_t nw = dr_dense_bits_words(rows);
  DR_REQUIRE(ceil_div(nw, 256) < kDcMaxN, DR_INVALID_ARGUMENT, "dense marks: too many rows");
  hipLaunchKernelGGL(dc_fill_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, s, bits, nw,
                     rows, all);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

}  // namespace dr

extern "C" {

int64_t dr_dense_bits_num_words(int64_t rows) { return dr_dense_bits_words(rows); }

int dr_dense_mark_rows(const dr_dense_mark_desc* descs, int num_tables, void* stream) {
  using namespace dr;
  DR_REQUIRE(num_tables >= 0, DR_INVALID_ARGUMENT, "dense mark: negative num_tables");
  DR_REQUIRE(descs || num_tables == 0, DR_INVALID_ARGUMENT, "dense mark: null descriptors");
  for (int t = 0; t < num_tables; ++t) {
    const dr_dense_mark_desc& d = descs[t];
    if (!d.bits) continue;
    DR_REQUIRE(d.rows >= 1 && d.n >= 0, DR_INVALID_ARGUMENT,
               "dense mark table %d: rows must be >= 1, n >= 0", t);
    DR_REQUIRE(d.n < kDcMaxN, DR_INVALID_ARGUMENT, "dense mark table %d: n >= 2^31 positions", t);
    DR_REQUIRE(d.n == 0 || d.idx, DR_INVALID_ARGUMENT, "dense mark table %d: null idx", t);
  }
  hipStream_t s = S(stream);
  int t = 0;
  while (t < num_tables) {
    DcMarkArgs a;
    memset(&a, 0, sizeof(a));
    int T = 0;
    for (; t < num_tables && T < DR_MAX_GROUP; ++t) {
      const dr_dense_mark_desc& d = descs[t];
      if (!d.bits || d.n == 0) continue;
      if (a.off[T] + d.n >= kDcMaxN) break;  // (every n < 2^31: T >= 1 here, the next launch takes it)
      DcMarkTable& o = a.t[T];
      o.bits = d.bits;
      o.idx = d.idx;
      o.n_dev = d.n_dev;
      o.n = d.n;
      o.rows = d.rows;
      a.off[T + 1] = a.off[T] + d.n;
      ++T;
    }
    if (T == 0) continue;  // (only skipped descriptors were passed over)
    hipLaunchKernelGGL(dc_mark_kernel, dim3((unsigned)ceil_div(a.off[T], 256)), dim3(256), 0, s, a,
                       T);
    DR_LAUNCH_CHECK();
  }
  return DR_OK;
}

int dr_dense_mark_all(uint32_t* bits, int64_t rows, void* stream) {
  return dr::dc_fill(bits, rows, 1, dr::S(stream));
}

int dr_dense_clear_marks(uint32_t* bits, int64_t rows, void* stream) {
  return dr::dc_fill(bits, rows, 0, dr::S(stream));
}

int dr_dense_marked_count(const uint32_t* bits, int64_t rows, int64_t* count_dev, void* stream) {
  using namespace dr;
  DR_REQUIRE(bits && count_dev, DR_INVALID_ARGUMENT, "dense count: null bits or count");
  DR_REQUIRE(rows >= 1, DR_INVALID_ARGUMENT, "dense count: rows must be >= 1");
  hipStream_t s = S(stream);
  int rc = fill_bytes(count_dev, 0, sizeof(int64_t), s);
  if (rc) return rc;
  const int64_t nw = dr_dense_bits_words(rows);
  const int64_t blocks = std::min<int64_t>(ceil_div(nw, 256), 1024);
  hipLaunchKernelGGL(dc_count_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bits, nw, rows,
                     reinterpret_cast<unsigned long long*>(count_dev));
  DR_LAUNCH_CHECK();
  return DR_OK;
}

size_t dr_dense_export_marked_workspace_size(int64_t rows) {
  return dr::carve_export(nullptr, rows).bytes;
}

int dr_dense_export_marked(const uint32_t* bits, int64_t rows, int dim, const float* const* cols,
                           int num_cols, int64_t capacity, int64_t* rows_out,
                           float* const* vals_out, int64_t* m_dev, void* ws, size_t ws_bytes,
                           void* stream) {
  using namespace dr;
  DR_REQUIRE(bits && m_dev, DR_INVALID_ARGUMENT, "dense export: null bits or m_dev");
  DR_REQUIRE(rows >= 1 && rows < kDcMaxN, DR_INVALID_ARGUMENT,
             "dense export: rows must be in [1, 2^31)");
  DR_REQUIRE(num_cols >= 0 && num_cols <= DR_DENSE_MAX_COLS, DR_INVALID_ARGUMENT,
             "dense export: %d columns (0 .. %d)", num_cols, DR_DENSE_MAX_COLS);
  DR_REQUIRE(capacity >= 0 && capacity < kDcMaxN, DR_INVALID_ARGUMENT,
             "dense export: capacity must be in [0, 2^31)");
  DR_REQUIRE(num_cols == 0 || (cols && (capacity == 0 || vals_out)), DR_INVALID_ARGUMENT,
             "dense export: null cols or vals_out");
  DR_REQUIRE(capacity == 0 || rows_out, DR_INVALID_ARGUMENT, "dense export: null rows_out");
  DcCols a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < num_cols; ++c) {
    DR_REQUIRE(cols[c] && (capacity == 0 || vals_out[c]), DR_INVALID_ARGUMENT,
               "dense export: column %d is null", c);
    a.src[c] = cols[c];
    a.dst[c] = capacity ? vals_out[c] : nullptr;
    DR_REQUIRE((const void*)a.src[c] != (const void*)a.dst[c], DR_INVALID_ARGUMENT,
               "dense export: column %d is exported onto itself", c);
  }
  const bool v4 = dc_v4(dim, a, num_cols);
  DR_REQUIRE(dc_dim_ok(dim, v4), DR_INVALID_ARGUMENT,
             "dense export: row width %d unsupported (max 1024 when a multiple of 4 and 16-byte "
             "aligned, else 256)", dim);
  DcExportWs w = carve_export(ws, rows);
  DR_REQUIRE(ws && ws_bytes >= w.bytes, DR_INVALID_ARGUMENT,
             "dense export: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0,
             w.bytes);
  hipStream_t s = S(stream);
  const int64_t nw = dr_dense_bits_words(rows);
  const dim3 grid((unsigned)ceil_div(nw, 256));
  hipLaunchKernelGGL(dc_popc_kernel, grid, dim3(256), 0, s, bits, nw, rows, w.cnt);
  DR_LAUNCH_CHECK();
  int rc = scan_exclusive_i32(w.cnt, w.pre, nw, nullptr, m_dev, w.scan_ws, s);
  if (rc) return rc;
  if (capacity == 0) return DR_OK;
  hipLaunchKernelGGL(dc_row_ids_kernel, grid, dim3(256), 0, s, bits, nw, rows, w.pre, capacity,
                     rows_out);
  DR_LAUNCH_CHECK();
  if (num_cols == 0) return DR_OK;
  return dispatch_dc_rows(false, v4, a, num_cols, rows, dim, rows_out, capacity, m_dev, nullptr,
                          s);
}

int dr_dense_upsert_rows(float* const* cols, int num_cols, int64_t rows, int dim,
                         const int64_t* idx, int64_t n, const int64_t* n_dev,
                         const float* const* vals, void* stream) {
  using namespace dr;
  DR_REQUIRE(num_cols >= 1 && num_cols <= DR_DENSE_MAX_COLS, DR_INVALID_ARGUMENT,
             "dense upsert: %d columns (1 .. %d)", num_cols, DR_DENSE_MAX_COLS);
  DR_REQUIRE(cols && vals, DR_INVALID_ARGUMENT, "dense upsert: null cols or vals");
  DR_REQUIRE(rows >= 1, DR_INVALID_ARGUMENT, "dense upsert: rows must be >= 1");
  DR_REQUIRE(n >= 0 && n < kDcMaxN, DR_INVALID_ARGUMENT, "dense upsert: n must be in [0, 2^31)");
  DR_REQUIRE(n == 0 || idx, DR_INVALID_ARGUMENT, "dense upsert: null idx");
  DcCols a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < num_cols; ++c) {
    DR_REQUIRE(cols[c] && (n == 0 || vals[c]), DR_INVALID_ARGUMENT,
               "dense upsert: column %d is null", c);
    a.src[c] = n ? vals[c] : nullptr;
    a.dst[c] = cols[c];
    DR_REQUIRE((const void*)a.src[c] != (const void*)a.dst[c], DR_INVALID_ARGUMENT,
               "dense upsert: column %d is written from itself", c);
    for (int u = 0; u < c; ++u)
      DR_REQUIRE(cols[u] != cols[c], DR_INVALID_ARGUMENT,
                 "dense upsert: columns %d and %d are the same block", u, c);
  }
  const bool v4 = dc_v4(dim, a, num_cols);
  DR_REQUIRE(dc_dim_ok(dim, v4), DR_INVALID_ARGUMENT,
             "dense upsert: row width %d unsupported (max 1024 when a multiple of 4 and 16-byte "
             "aligned, else 256)", dim);
  if (n == 0) return DR_OK;
  int* st = status_word();
  DR_REQUIRE(st, DR_INTERNAL, "status word unavailable");
  return dispatch_dc_rows(true, v4, a, num_cols, rows, dim, idx, n, n_dev, st, S(stream));
}

}  // extern "C"
