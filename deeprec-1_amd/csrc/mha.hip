// mha.hip -- multi-head self-attention over a padded history, forward and
// backward, one launch each, fp32 on the matrix cores.
//
// For sample b with L = clamp(seq_len[b], 0, T), head h, query t < L:
//   s[j] = scale * dot(q[b,t,h,:], k[b,j,h,:])   (j < L)      p = softmax_j(s)
//   out[b,t,h,:] = sum_j p[j] v[b,j,h,:]          saved[b,h,t] = logsumexp_j(s)
// and exact zeros at t >= L (the reference's key masking, then query masking).
//
// Mapping: one wave owns one (sample, head) for the whole launch; the four
// waves of a block share nothing and never synchronise.  Keys and queries are
// cut into tiles of 16 and only the tiles below ceil(L / 16) are visited; a
// row index past L - 1 inside the last tile reads row L - 1 (in range, finite)
// and is masked.  Every product is v_mfma_f32_16x16x4_f32:
//   * a "row fragment" of a [16, HD] tile gives lane (r, g) = (lane % 16,
//     lane / 16) the VEC consecutive floats d = j * 4 VEC + VEC g + c of row r
//     as one 8 / 16-byte load; component (j, c) is contraction step j VEC + c,
//     where the lane supplies k-slot g.  The A and B operand of the MFMA have
//     the same lane map, so one fragment serves either side and swapping the
//     operands transposes the product;
//   * the strip is computed transposed, S^T = K Q^T: accumulator register i
//     of lane (r, g) is key 4 g + i, query r.  The softmax over keys is then
//     over a lane's own registers and two xor steps (16, 32), and register i
//     is already the A operand (query r, k-slot g) of the P V product whose B
//     operand holds V rows 4 g + i ("column fragment": lane (r, g), register
//     i = X[4 g + i][16 n + r]).  The probabilities never leave the registers.
// The head's K and V fragments are loaded once and stay in registers.
//
// Backward needs the strip in both orientations (grad_q contracts over keys,
// grad_k and grad_v over queries) and forms each with its own MFMAs rather
// than transposing through LDS; grad_k and grad_v accumulate in registers
// over the query tiles and are stored once.  No atomics, no LDS, no scratch.
#include <math.h>

#include "dr_common.h"

namespace dr {
namespace {

constexpr int MHA_WAVES = 4;    // (sample, head) pairs per block
constexpr int MHA_MAX_T = 128;
constexpr int MHA_KT = MHA_MAX_T / 16;

typedef float mf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ mf4 mma(float a, float b, mf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int HD>
struct Shape {
  static constexpr int VEC = HD >= 16 ? 4 : 2;      // floats per fragment load
  static constexpr int NV = HD / (4 * VEC);         // fragment loads per row
  static constexpr int NC = HD / 4;                 // contraction steps over head_dim
  static constexpr int NT = (HD + 15) / 16;         // 16-column output tiles
};

// Row fragment of the row at p (the head's first column): steps j VEC + c.
template <int HD>
__device__ __forceinline__ void row_frag(const float* p, int g, float (&f)[Shape<HD>::NC]) {
  using S = Shape<HD>;
#pragma unroll
  for (int j = 0; j < S::NV; ++j) {
    if constexpr (S::VEC == 4) {
      const float4 x = gld(reinterpret_cast<const float4*>(p + j * 16 + 4 * g));
      f[4 * j] = x.x, f[4 * j + 1] = x.y, f[4 * j + 2] = x.z, f[4 * j + 3] = x.w;
    } else {
      const float2 x = gld(reinterpret_cast<const float2*>(p + j * 8 + 2 * g));
      f[2 * j] = x.x, f[2 * j + 1] = x.y;
    }
  }
}

// Column fragment of the 16 rows from row0: f[n][i] = X[row0 + 4 g + i][16 n + r],
// rows clamped to last, columns past HD zero (HD = 8: half a tile is padding).
template <int HD>
__device__ __forceinline__ void col_frag(const float* base, int64_t ld, int row0, int last, int r,
                                         int g, float (&f)[Shape<HD>::NT][4]) {
#pragma unroll
  for (int n = 0; n < Shape<HD>::NT; ++n) {
    const int col = 16 * n + r;
    const bool on = col < HD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = row0 + 4 * g + i;
      row = row < last ? row : last;
      const float x = gld(base + (int64_t)row * ld + (on ? col : 0));
      f[n][i] = on ? x : 0.0f;
    }
  }
}

__device__ __forceinline__ float xor_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 16, 64));
  return fmaxf(x, __shfl_xor(x, 32, 64));
}
__device__ __forceinline__ float xor_sum(float x) {
  x += __shfl_xor(x, 16, 64);
  return x + __shfl_xor(x, 32, 64);
}

// Rows [from, T) of the head's HD columns (row stride ld, 16-byte aligned) = 0.
template <int HD>
__device__ __forceinline__ void zero_rows(float* base, int64_t ld, int from, int T, int lane) {
  constexpr int Q = HD / 4;
  const int n = (T - from) * Q;
  for (int e = lane; e < n; e += 64) {
    const int row = from + e / Q, c = e % Q;
    gst(reinterpret_cast<float4*>(base + (int64_t)row * ld + 4 * c),
        make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

// Tile (16 rows from row0) of accumulators acc[n][i] = X[row0 + 4 g + i][16 n + r]
// times mul, rows below L only.
template <int HD>
__device__ __forceinline__ void store_tile(float* base, int64_t ld, int row0, int L, int r, int g,
                                           const mf4 (&acc)[Shape<HD>::NT], float mul) {
#pragma unroll
  for (int n = 0; n < Shape<HD>::NT; ++n) {
    const int col = 16 * n + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 4 * g + i;
      if (row < L && col < HD) gst(base + (int64_t)row * ld + col, acc[n][i] * mul);
    }
  }
}

struct Who {
  int64_t b;
  int h, L, lane, r, g;
};

// The wave's (sample, head) and clamped length; false for an idle wave.
__device__ __forceinline__ bool who(const int32_t* seq_len, int64_t B, int T, int heads, Who& w) {
  w.lane = threadIdx.x & 63;
  w.r = w.lane & 15, w.g = w.lane >> 4;
  const int64_t pair = (int64_t)blockIdx.x * MHA_WAVES + (threadIdx.x >> 6);
  if (pair >= B * heads) return false;
  w.b = pair / heads;
  w.h = (int)(pair - w.b * heads);
  int n = __builtin_amdgcn_readfirstlane(gld(seq_len + w.b));
  w.L = n < 0 ? 0 : (n > T ? T : n);
  return true;
}

template <int HD>
__global__ __launch_bounds__(MHA_WAVES * 64) void mha_forward_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    int64_t ld, const int32_t* __restrict__ seq_len, int64_t B, int T, int heads, float scale,
    float* __restrict__ out, float* __restrict__ saved) {
  using S = Shape<HD>;
  Who w;
  if (!who(seq_len, B, T, heads, w)) return;
  const int L = w.L, r = w.r, g = w.g, lane = w.lane;
  const int64_t E = (int64_t)heads * HD;
  const int64_t in0 = w.b * T * ld + w.h * HD;           // the head's first input element
  float* ob = out + w.b * T * E + w.h * HD;
  float* sb = saved + (w.b * heads + w.h) * T;
  zero_rows<HD>(ob, E, L, T, lane);
  for (int t = L + lane; t < T; t += 64) gst(sb + t, 0.0f);
  if (L == 0) return;
  const int nt = (L + 15) >> 4, last = L - 1;

  float kf[MHA_KT][S::NC], vf[MHA_KT][S::NT][4];
#pragma unroll
  for (int kt = 0; kt < MHA_KT; ++kt) {
    if (kt < nt) {
      const int row = kt * 16 + r < last ? kt * 16 + r : last;
      row_frag<HD>(k + in0 + (int64_t)row * ld, g, kf[kt]);
      col_frag<HD>(v + in0, ld, kt * 16, last, r, g, vf[kt]);
    }
  }

  float qf[S::NC], qn[S::NC];
  row_frag<HD>(q + in0 + (int64_t)(r < last ? r : last) * ld, g, qf);
  for (int qt = 0; qt < nt; ++qt) {
    {  // the next tile's Q before this tile's products (the last tile re-reads itself)
      const int t = (qt + 1 < nt ? qt + 1 : qt) * 16 + r;
      row_frag<HD>(q + in0 + (int64_t)(t < last ? t : last) * ld, g, qn);
    }
    mf4 st[MHA_KT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < MHA_KT; ++kt) {
      if (kt < nt) {
        mf4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < S::NC; ++s) a = mma(kf[kt][s], qf[s], a);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = kt * 16 + 4 * g + i < L ? a[i] * scale : -INFINITY;
          m = fmaxf(m, a[i]);
        }
        st[kt] = a;
      }
    }
    m = xor_max(m);                      // key 0 is valid: m is finite
    float sum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < MHA_KT; ++kt) {
      if (kt < nt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          st[kt][i] = __expf(st[kt][i] - m);
          sum += st[kt][i];
        }
      }
    }
    sum = xor_sum(sum);
    const float inv = 1.0f / sum;
    mf4 o[S::NT];
#pragma unroll
    for (int n = 0; n < S::NT; ++n) o[n] = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < MHA_KT; ++kt) {
      if (kt < nt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = st[kt][i] * inv;
#pragma unroll
          for (int n = 0; n < S::NT; ++n) o[n] = mma(p, vf[kt][n][i], o[n]);
        }
      }
    }
    store_tile<HD>(ob, E, qt * 16, L, r, g, o, 1.0f);
    if (g == 0 && qt * 16 + r < L) gst(sb + qt * 16 + r, m + logf(sum));
#pragma unroll
    for (int s = 0; s < S::NC; ++s) qf[s] = qn[s];
  }
}

template <int HD>
__global__ __launch_bounds__(MHA_WAVES * 64) void mha_backward_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    int64_t ld, const int32_t* __restrict__ seq_len, const float* __restrict__ out,
    const float* __restrict__ saved, const float* __restrict__ grad_out, int64_t B, int T,
    int heads, float scale, float* __restrict__ grad_q, float* __restrict__ grad_k,
    float* __restrict__ grad_v, int64_t ldg) {
  using S = Shape<HD>;
  Who w;
  if (!who(seq_len, B, T, heads, w)) return;
  const int L = w.L, r = w.r, g = w.g, lane = w.lane;
  const int64_t E = (int64_t)heads * HD;
  const int64_t in0 = w.b * T * ld + w.h * HD;
  const int64_t o0 = w.b * T * E + w.h * HD;             // out / grad_out (contiguous)
  const int64_t g0 = w.b * T * ldg + w.h * HD;
  const float* sb = saved + (w.b * heads + w.h) * T;
  zero_rows<HD>(grad_q + g0, ldg, L, T, lane);
  zero_rows<HD>(grad_k + g0, ldg, L, T, lane);
  zero_rows<HD>(grad_v + g0, ldg, L, T, lane);
  if (L == 0) return;
  const int nt = (L + 15) >> 4, last = L - 1;

  // the head's K and V as row fragments (both strip orientations), K as
  // column fragments (grad_q's B operand), and the two accumulators
  // (head_dim 32: declared resident they spill beside the accumulators; read
  // inside the pair loop they are the compiler's to keep or re-read, from cache)
  constexpr bool KV_REGS = HD <= 16;
  constexpr int KV = KV_REGS ? MHA_KT : 1;
  float kf[KV][S::NC], vf[KV][S::NC], kc[KV][S::NT][4];
  mf4 gk[MHA_KT][S::NT], gv[MHA_KT][S::NT];
  auto load_kv = [&](int kt, int at) {
    const int row = kt * 16 + r < last ? kt * 16 + r : last;
    row_frag<HD>(k + in0 + (int64_t)row * ld, g, kf[at]);
    row_frag<HD>(v + in0 + (int64_t)row * ld, g, vf[at]);
    col_frag<HD>(k + in0, ld, kt * 16, last, r, g, kc[at]);
  };
#pragma unroll
  for (int kt = 0; kt < MHA_KT; ++kt) {
    if constexpr (KV_REGS)
      if (kt < nt) load_kv(kt, kt);
#pragma unroll
    for (int n = 0; n < S::NT; ++n) gk[kt][n] = gv[kt][n] = mf4{0.f, 0.f, 0.f, 0.f};
  }

  for (int qt = 0; qt < nt; ++qt) {
    const int tr = qt * 16 + r < last ? qt * 16 + r : last;   // the lane's query as a column
    float qf[S::NC], df[S::NC], of[S::NC];
    row_frag<HD>(q + in0 + (int64_t)tr * ld, g, qf);
    row_frag<HD>(grad_out + o0 + (int64_t)tr * E, g, df);
    row_frag<HD>(out + o0 + (int64_t)tr * E, g, of);
    float qc[S::NT][4], dc[S::NT][4];
    col_frag<HD>(q + in0, ld, qt * 16, last, r, g, qc);
    col_frag<HD>(grad_out + o0, E, qt * 16, last, r, g, dc);
    const float lse_r = gld(sb + tr);
    float lse_i[4], D_i[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = qt * 16 + 4 * g + i;
      lse_i[i] = gld(sb + (t < last ? t : last));
    }
    float D_r = 0.0f;                    // D of query r: a lane's part, then the four k-slots
#pragma unroll
    for (int s = 0; s < S::NC; ++s) D_r += df[s] * of[s];
    D_r = xor_sum(D_r);
#pragma unroll
    for (int i = 0; i < 4; ++i) D_i[i] = __shfl(D_r, 4 * g + i, 64);
    const bool qr_on = qt * 16 + r < L;

    mf4 gq[S::NT];
#pragma unroll
    for (int n = 0; n < S::NT; ++n) gq[n] = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < MHA_KT; ++kt) {
      if (kt < nt) {
        // keys in rows: register i = key 4 g + i, query r -> grad_q (over keys)
        if constexpr (!KV_REGS) load_kv(kt, 0);
        constexpr int at_ = 0;
        const int at = KV_REGS ? kt : at_;
        mf4 a = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < S::NC; ++s) {
          a = mma(kf[at][s], qf[s], a);
          d = mma(vf[at][s], df[s], d);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool on = qr_on && kt * 16 + 4 * g + i < L;
          const float p = on ? __expf(a[i] * scale - lse_r) : 0.0f;
          const float ds = p * (d[i] - D_r);
#pragma unroll
          for (int n = 0; n < S::NT; ++n) gq[n] = mma(ds, kc[at][n][i], gq[n]);
        }
        // queries in rows: register i = query 4 g + i, key r -> grad_k, grad_v (over queries)
        a = mf4{0.f, 0.f, 0.f, 0.f}, d = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < S::NC; ++s) {
          a = mma(qf[s], kf[at][s], a);
          d = mma(df[s], vf[at][s], d);
        }
        const bool kr_on = kt * 16 + r < L;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool on = kr_on && qt * 16 + 4 * g + i < L;
          const float p = on ? __expf(a[i] * scale - lse_i[i]) : 0.0f;
          const float ds = p * (d[i] - D_i[i]);
#pragma unroll
          for (int n = 0; n < S::NT; ++n) {
            gv[kt][n] = mma(p, dc[n][i], gv[kt][n]);
            gk[kt][n] = mma(ds, qc[n][i], gk[kt][n]);
          }
        }
      }
    }
    store_tile<HD>(grad_q + g0, ldg, qt * 16, L, r, g, gq, scale);
  }
#pragma unroll
  for (int kt = 0; kt < MHA_KT; ++kt) {
    if (kt < nt) {
      store_tile<HD>(grad_k + g0, ldg, kt * 16, L, r, g, gk[kt], scale);
      store_tile<HD>(grad_v + g0, ldg, kt * 16, L, r, g, gv[kt], 1.0f);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int mha_check(const char* what, int64_t B, int64_t T, int64_t heads, int64_t hd, int64_t ld,
              int64_t ldg) {
  DR_REQUIRE(hd == 8 || hd == 16 || hd == 32, DR_INVALID_ARGUMENT,
             "%s (mha): head_dim %lld has no kernel shape (8, 16 or 32)", what, (long long)hd);
  DR_REQUIRE(heads >= 1 && heads <= (1 << 16), DR_INVALID_ARGUMENT,
             "%s (mha): heads %lld is outside [1, 2^16]", what, (long long)heads);
  DR_REQUIRE(T >= 1 && T <= MHA_MAX_T, DR_INVALID_ARGUMENT,
             "%s (mha): seq_len %lld is outside [1, %d]", what, (long long)T, MHA_MAX_T);
  DR_REQUIRE(B >= 0 && B * heads <= (int64_t(1) << 31) - 1, DR_INVALID_ARGUMENT,
             "%s (mha): batch %lld x heads %lld is outside [0, 2^31)", what, (long long)B,
             (long long)heads);
  DR_REQUIRE(ld >= heads * hd && ldg >= heads * hd, DR_INVALID_ARGUMENT,
             "%s (mha): row stride %lld / %lld is below heads * head_dim = %lld", what,
             (long long)ld, (long long)ldg, (long long)(heads * hd));
  DR_REQUIRE(ld % 4 == 0 && ldg % 4 == 0, DR_INVALID_ARGUMENT,
             "%s (mha): row stride %lld / %lld is not a multiple of 4 floats", what, (long long)ld,
             (long long)ldg);
  return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" size_t dr_mha_seq_saved_size(int64_t B, int64_t T, int64_t heads) {
  if (B <= 0 || T <= 0 || heads <= 0) return 0;
  return (size_t)B * (size_t)heads * (size_t)T * sizeof(float);
}

extern "C" int dr_mha_seq_forward(const float* q, const float* k, const float* v, int64_t ld,
                                  const int32_t* seq_len, int64_t B, int64_t T, int64_t heads,
                                  int64_t head_dim, float scale, float* out, float* saved,
                                  void* stream) {
  const char* what = "dr_mha_seq_forward";
  if (int rc = mha_check(what, B, T, heads, head_dim, ld, heads * head_dim)) return rc;
  DR_REQUIRE(q && k && v && seq_len && out && saved, DR_INVALID_ARGUMENT,
             "%s (mha): a required pointer is null", what);
  DR_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), DR_INVALID_ARGUMENT,
             "%s (mha): q, k, v and out must be 16-byte aligned", what);
  if (B == 0) return DR_OK;
  const dim3 grid((unsigned)ceil_div(B * heads, MHA_WAVES)), block(MHA_WAVES * 64);
#define DR_MHA_FWD(HD)                                                                         \
  hipLaunchKernelGGL(mha_forward_kernel<HD>, grid, block, 0, S(stream), q, k, v, ld, seq_len, B, \
                     (int)T, (int)heads, scale, out, saved)
  if (head_dim == 8) DR_MHA_FWD(8);
  else if (head_dim == 16) DR_MHA_FWD(16);
  else DR_MHA_FWD(32);
#undef DR_MHA_FWD
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_mha_seq_backward(const float* q, const float* k, const float* v, int64_t ld,
                                   const int32_t* seq_len, const float* out, const float* saved,
                                   const float* grad_out, int64_t B, int64_t T, int64_t heads,
                                   int64_t head_dim, float scale, float* grad_q, float* grad_k,
                                   float* grad_v, int64_t ld_grad, void* stream) {
  const char* what = "dr_mha_seq_backward";
  if (int rc = mha_check(what, B, T, heads, head_dim, ld, ld_grad)) return rc;
  DR_REQUIRE(q && k && v && seq_len && out && saved && grad_out && grad_q && grad_k && grad_v,
             DR_INVALID_ARGUMENT, "%s (mha): a required pointer is null", what);
  DR_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) &&
                 aligned16(grad_out) && aligned16(grad_q) && aligned16(grad_k) && aligned16(grad_v),
             DR_INVALID_ARGUMENT,
             "%s (mha): q, k, v, out, grad_out and the gradients must be 16-byte aligned", what);
  if (B == 0) return DR_OK;
  const dim3 grid((unsigned)ceil_div(B * heads, MHA_WAVES)), block(MHA_WAVES * 64);
#define DR_MHA_BWD(HD)                                                                          \
  hipLaunchKernelGGL(mha_backward_kernel<HD>, grid, block, 0, S(stream), q, k, v, ld, seq_len,  \
                     out, saved, grad_out, B, (int)T, (int)heads, scale, grad_q, grad_k, grad_v, \
                     ld_grad)
  if (head_dim == 8) DR_MHA_BWD(8);
  else if (head_dim == 16) DR_MHA_BWD(16);
  else DR_MHA_BWD(32);
#undef DR_MHA_BWD
  DR_LAUNCH_CHECK();
  return DR_OK;
}
