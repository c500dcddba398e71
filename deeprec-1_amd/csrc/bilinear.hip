// bilinear.hip -- FiBiNET's bilinear interaction over every pair of fields,
// forward and backward, fp32 on the matrix cores.
//
//   v[b, i, :] = x[b, i, :]  or  scale[b, i] x[b, i, :]
//   out[b, p(i, j), d] = (sum_k v[b, i, k] W[sel, k, d]) v[b, j, d]      i < j
//
// p(i, j) is the row-major upper-triangle index and sel is 0, i or p for kind
// all, each or interaction.  Every product is v_mfma_f32_16x16x4_f32 with the
// SAMPLES as columns: lane (r, g) = (lane % 16, lane / 16) supplies A[row r]
// [k g] and B[k g][column r], and accumulator register c of the lane is
// element [4 g + c][r].  With the rows a 16-wide panel of d, the lane holds
// four consecutive d of sample r: u = v W, the incoming gradient, v_j and the
// output all meet in that layout as 16-byte loads and stores, and an
// accumulator is at once the B operand of the next product (step (panel, c)
// gives k slot g the element 16 panel + 4 g + c, which is what register c
// holds), so gu W^T follows gu without a trip through LDS.  A column is one
// sample from end to end: nothing a sample gets depends on its neighbours.
//
// A tile is 16 samples.  A block of 8 waves stages the tile's v (scaled on the
// way in, rows padded to 16 floats with zeros) in LDS once and each wave takes
// one field of it; when 16 m ceil16(D) floats pass 64 KB the waves read x and
// scale from global memory instead (same arithmetic, same bits).  Reads past
// D, past m or past B are predicated, never padded copies.
//
// Forward (one launch): the wave of field i forms u_i once (all, each) or
// u_ij per pair (interaction) and walks j > i: out = u * v_j, one 16-byte
// store a lane, 64 contiguous bytes or more a sample.
//
// Input gradients (one launch): the wave of field f owns grad_x[:, f, :] and
// grad_scale[:, f] whole, in both of the field's roles, so nothing is
// accumulated across waves: as i it sums gu = sum_j g_fj * v_j and adds
// gu W_f^T (interaction: (g_fj * v_j) W_fj^T per pair, each pair a chain of
// its own); as j it adds g_if * u_i for i < f with u recomputed.  Every field
// has m - 1 pairs to visit.  grad_out is read twice this way, once per role.
//
// Weight gradient (one launch and a finishing launch): a wave owns one weight
// matrix (a field, or a pair) and one of S slices of the tiles, and walks its
// slice: lane (r, g) forms gu[sample 4 s + g][d 16 panel + r] elementwise,
// which is the B operand of gW += v_i^T gu with the samples as K (the third
// and last read of grad_out; DESIGN section 31 on fusing it away).  The chain
// is cut every 16 tiles.  S is fixed by (B, m, D, kind) and falls as W grows
// (64 MiB of partials at most); the finishing kernel adds the partials in
// a fixed order (16 strided sums a matrix element, then those in order; kind
// all: over slices and fields).  No atomics anywhere.
#include "dr_common.h"

namespace dr {
namespace {

constexpr int BL_MAX_M = 64, BL_MAX_D = 64, BL_MAX_DP = BL_MAX_D / 16;
constexpr int BL_THREADS = 512, BL_WAVES = BL_THREADS / 64;
constexpr int64_t BL_MAX_B = (int64_t(1) << 31) - 1;
constexpr int BL_LDS_FLOATS = 16384;              // v of a tile in LDS up to 64 KB
constexpr int BL_MAX_SLICES = 256, BL_WG_WAVES = 8192, BL_CHAIN_TILES = 16;
constexpr size_t BL_MAX_PARTIAL_BYTES = size_t(64) << 20;
enum { BL_ALL = 0, BL_EACH = 1, BL_INTERACTION = 2 };

typedef float mf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ mf4 mma(float a, float b, mf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__host__ __device__ __forceinline__ int pair_index(int i, int j, int m) {
  return i * (2 * m - i - 1) / 2 + j - i - 1;
}

// p[d0 .. d0 + 3] with zeros at and past D; vec: D is a multiple of 4 and p is
// 16-byte aligned.
__device__ __forceinline__ mf4 ld4(const float* p, int d0, int D, bool vec) {
  mf4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if (d0 < D) v = gld(reinterpret_cast<const mf4*>(p + d0));
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (d0 + c < D) v[c] = gld(p + d0 + c);
  }
  return v;
}
__device__ __forceinline__ void st4(float* p, int d0, int D, bool vec, mf4 v) {
  if (vec) {
    if (d0 < D) gst(reinterpret_cast<mf4*>(p + d0), v);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (d0 + c < D) gst(p + d0 + c, v[c]);
  }
}

// The tile's v as lane (r, g) sees it: sample r's row of a field.
template <bool LDSV>
struct VTile {
  const float* row;     // LDSV: the sample's strip in LDS, fields FS floats apart
  const float* xb;      // x + b m D
  const float* sb;      // scale + b m, or null
  int D, FS;
  bool vec;
  __device__ __forceinline__ mf4 at(int field, int d0) const {
    if (LDSV) return *reinterpret_cast<const mf4*>(row + field * FS + d0);
    mf4 v = ld4(xb + field * D, d0, D, vec);
    if (sb != nullptr) v = v * gld(sb + field);
    return v;
  }
};

// Sample stride of the staged tile: m FS floats and 4 more, so that the 16
// samples' 16-byte reads of one field spread over the banks.
__host__ __device__ __forceinline__ int tile_stride(int m, int D) {
  return m * (((D + 15) >> 4) * 16) + 4;
}

// Stage the tile's v: [sample][field][FS] with zeros past D, rows past B a
// copy of the last sample (they are never stored).
__device__ __forceinline__ void stage_tile(float* lds, const float* x, const float* scale,
                                           int64_t b0, int64_t B, int m, int D) {
  const int FS = ((D + 15) >> 4) * 16, SS = tile_stride(m, D), per = m * FS;
  for (int e = threadIdx.x; e < 16 * per; e += BL_THREADS) {
    const int smp = e / per, rem = e - smp * per, field = rem / FS, d = rem - field * FS;
    const int64_t b = b0 + smp < B ? b0 + smp : B - 1;
    float v = 0.0f;
    if (d < D) {
      v = gld(x + (b * m + field) * D + d);
      if (scale != nullptr) v = v * gld(scale + b * m + field);
    }
    lds[smp * SS + rem] = v;
  }
}

// u[panel] (register c: d = 16 panel + 4 g + c of sample r) = v_field W, W one
// [D, D] matrix.  Step (kp, c) gives k slot g the element k = 16 kp + 4 g + c.
template <bool LDSV>
__device__ __forceinline__ void form_u(const VTile<LDSV>& vt, int field, const float* W, int D,
                                       int DP, int r, int g, mf4* u) {
#pragma unroll
  for (int dp = 0; dp < BL_MAX_DP; ++dp) u[dp] = mf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kp = 0; kp < BL_MAX_DP; ++kp) {
    if (kp < DP) {
      const mf4 vb = vt.at(field, 16 * kp + 4 * g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 16 * kp + 4 * g + c;
#pragma unroll
        for (int dp = 0; dp < BL_MAX_DP; ++dp) {
          if (dp < DP) {
            const int d = 16 * dp + r;
            const float a = k < D && d < D ? gld(W + k * D + d) : 0.0f;
            u[dp] = mma(a, vb[c], u[dp]);
          }
        }
      }
    }
  }
}

// acc[kp] (register c: k = 16 kp + 4 g + c of sample r) += gu W^T, the
// product a chain of its own.  Step (dp, c) gives k slot g the element
// d = 16 dp + 4 g + c, register c of gu[dp].
__device__ __forceinline__ void add_gu_wt(const mf4* gu, const float* W, int D, int DP, bool vec,
                                          int r, int g, mf4* acc) {
#pragma unroll
  for (int kp = 0; kp < BL_MAX_DP; ++kp) {
    if (kp < DP) {
      const int k = 16 * kp + r;
      mf4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dp = 0; dp < BL_MAX_DP; ++dp) {
        if (dp < DP) {
          mf4 a = {0.f, 0.f, 0.f, 0.f};
          if (k < D) a = ld4(W + k * D, 16 * dp + 4 * g, D, vec);
#pragma unroll
          for (int c = 0; c < 4; ++c) t = mma(a[c], gu[dp][c], t);
        }
      }
      acc[kp] += t;
    }
  }
}

template <bool LDSV>
__global__ __launch_bounds__(BL_THREADS) void bilinear_forward_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ W,
    int kind, int64_t B, int m, int D, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int DP = (D + 15) >> 4, P = m * (m - 1) / 2, DD = D * D;
  const bool vec = (D & 3) == 0;
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  if (LDSV) {
    stage_tile(lds, x, scale, b0, B, m, D);
    __syncthreads();
  }
  const int i = blockIdx.y * BL_WAVES + wave;
  if (i >= m - 1) return;
  const bool on = b0 + r < B;
  const int64_t b = on ? b0 + r : B - 1;
  VTile<LDSV> vt;
  vt.row = lds + r * tile_stride(m, D);
  vt.xb = x + b * m * D;
  vt.sb = scale != nullptr ? scale + b * m : nullptr;
  vt.D = D;
  vt.FS = DP * 16;
  vt.vec = vec;

  mf4 u[BL_MAX_DP];
  if (kind != BL_INTERACTION) form_u(vt, i, W + (kind == BL_EACH ? (int64_t)i * DD : 0), D, DP, r, g, u);
  float* ob = out + b * P * D;
  for (int j = i + 1; j < m; ++j) {
    const int p = pair_index(i, j, m);
    if (kind == BL_INTERACTION) form_u(vt, i, W + (int64_t)p * DD, D, DP, r, g, u);
#pragma unroll
    for (int dp = 0; dp < BL_MAX_DP; ++dp) {
      if (dp < DP) {
        const int d0 = 16 * dp + 4 * g;
        const mf4 o = u[dp] * vt.at(j, d0);
        if (on) st4(ob + (int64_t)p * D, d0, D, vec, o);
      }
    }
  }
}

template <bool LDSV>
__global__ __launch_bounds__(BL_THREADS) void bilinear_input_grad_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ W,
    const float* __restrict__ go, int kind, int64_t B, int m, int D, float* __restrict__ gx,
    float* __restrict__ gscale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int DP = (D + 15) >> 4, P = m * (m - 1) / 2, DD = D * D;
  const bool vec = (D & 3) == 0;
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  if (LDSV) {
    stage_tile(lds, x, scale, b0, B, m, D);
    __syncthreads();
  }
  const int f = blockIdx.y * BL_WAVES + wave;
  if (f >= m) return;
  const bool on = b0 + r < B;
  const int64_t b = on ? b0 + r : B - 1;
  VTile<LDSV> vt;
  vt.row = lds + r * tile_stride(m, D);
  vt.xb = x + b * m * D;
  vt.sb = scale != nullptr ? scale + b * m : nullptr;
  vt.D = D;
  vt.FS = DP * 16;
  vt.vec = vec;
  const float* gb = go + b * P * D;

  mf4 gv[BL_MAX_DP], gu[BL_MAX_DP], u[BL_MAX_DP];
#pragma unroll
  for (int dp = 0; dp < BL_MAX_DP; ++dp) gv[dp] = gu[dp] = mf4{0.f, 0.f, 0.f, 0.f};

  // the field as j: gv += g_if * u_i
  for (int i = 0; i < f; ++i) {
    const int p = pair_index(i, f, m);
    const int sel = kind == BL_ALL ? 0 : kind == BL_EACH ? i : p;
    form_u(vt, i, W + (int64_t)sel * DD, D, DP, r, g, u);
#pragma unroll
    for (int dp = 0; dp < BL_MAX_DP; ++dp)
      if (dp < DP) gv[dp] += ld4(gb + (int64_t)p * D, 16 * dp + 4 * g, D, vec) * u[dp];
  }
  // the field as i: gu = sum_j g_fj * v_j, gv += gu W^T (interaction: per pair)
  for (int j = f + 1; j < m; ++j) {
    const int p = pair_index(f, j, m);
#pragma unroll
    for (int dp = 0; dp < BL_MAX_DP; ++dp) {
      if (dp < DP) {
        const int d0 = 16 * dp + 4 * g;
        const mf4 t = ld4(gb + (int64_t)p * D, d0, D, vec) * vt.at(j, d0);
        if (kind == BL_INTERACTION) gu[dp] = t;
        else gu[dp] += t;
      }
    }
    if (kind == BL_INTERACTION) add_gu_wt(gu, W + (int64_t)p * DD, D, DP, vec, r, g, gv);
  }
  if (kind != BL_INTERACTION && f < m - 1)
    add_gu_wt(gu, W + (kind == BL_EACH ? (int64_t)f * DD : 0), D, DP, vec, r, g, gv);

  // grad_x = a gv, grad_scale = sum_d gv x (over the lane's d, then over g)
  const float a = vt.sb != nullptr ? gld(vt.sb + f) : 1.0f;
  float part = 0.0f;
#pragma unroll
  for (int dp = 0; dp < BL_MAX_DP; ++dp) {
    if (dp < DP) {
      const int d0 = 16 * dp + 4 * g;
      if (gscale != nullptr) {
        const mf4 xv = ld4(vt.xb + f * D, d0, D, vec);
#pragma unroll
        for (int c = 0; c < 4; ++c) part += gv[dp][c] * xv[c];
      }
      if (on) st4(gx + (b * m + f) * D, d0, D, vec, gv[dp] * a);
    }
  }
  if (gscale != nullptr) {
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (on && g == 0) gst(gscale + b * m + f, part);
  }
}

struct WgPlan {
  int Q;          // weight matrices with a partial: fields (all: m - 1, each: m) or pairs
  int slices;
  int64_t tiles;
};

WgPlan wg_plan(int kind, int64_t B, int64_t m, int64_t D) {
  WgPlan p;
  p.Q = kind == BL_ALL ? (int)m - 1 : kind == BL_EACH ? (int)m : (int)(m * (m - 1) / 2);
  p.tiles = ceil_div(B, 16);
  int64_t S = BL_WG_WAVES / p.Q;
  if (S > BL_MAX_SLICES) S = BL_MAX_SLICES;
  if (S > p.tiles) S = p.tiles;
  while (S > 1 && (size_t)S * p.Q * D * D * sizeof(float) > BL_MAX_PARTIAL_BYTES) --S;
  p.slices = S < 1 ? 1 : (int)S;
  return p;
}

__global__ __launch_bounds__(64) void bilinear_weight_grad_kernel(
    const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ go,
    int kind, int64_t B, int m, int D, int64_t tiles, float* __restrict__ ws) {
  const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int DP = (D + 15) >> 4, P = m * (m - 1) / 2, q = blockIdx.x;
  int i = q, j_lo = q + 1, j_hi = m;                 // a field and every later one
  if (kind == BL_INTERACTION) {                      // or the pair q alone
    i = 0;
    while (q >= pair_index(i + 1, i + 2, m) && i + 2 < m) ++i;
    j_lo = i + 1 + q - pair_index(i, i + 1, m);
    j_hi = j_lo + 1;
  }
  const int64_t per = ceil_div(tiles, gridDim.y), first = blockIdx.y * per;
  const int64_t last = first + per < tiles ? first + per : tiles;

  mf4 acc[BL_MAX_DP][BL_MAX_DP], tot[BL_MAX_DP][BL_MAX_DP];
#pragma unroll
  for (int kp = 0; kp < BL_MAX_DP; ++kp)
#pragma unroll
    for (int dp = 0; dp < BL_MAX_DP; ++dp) acc[kp][dp] = tot[kp][dp] = mf4{0.f, 0.f, 0.f, 0.f};

  for (int64_t t = first; t < last; ++t) {
    // step s of the product: k slot g is sample 4 s + g; the four steps' loads go together
    const float *xb[4], *sb[4], *gb[4];
    float gu[4][BL_MAX_DP], av[4][BL_MAX_DP];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t bs = t * 16 + 4 * s + g;
      const bool live = bs < B;
      const int64_t b = live ? bs : B - 1;
      xb[s] = x + b * m * D;
      sb[s] = scale != nullptr ? scale + b * m : nullptr;
      gb[s] = go + b * P * D;
#pragma unroll
      for (int dp = 0; dp < BL_MAX_DP; ++dp) {
        const int d = 16 * dp + r;
        gu[s][dp] = av[s][dp] = 0.0f;
        if (dp < DP && d < D && live) {
          av[s][dp] = gld(xb[s] + i * D + d);
          if (sb[s] != nullptr) av[s][dp] = av[s][dp] * gld(sb[s] + i);
        }
      }
    }
    for (int j = j_lo; j < j_hi; ++j) {
      const int p = pair_index(i, j, m);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float aj = sb[s] != nullptr ? gld(sb[s] + j) : 1.0f;
#pragma unroll
        for (int dp = 0; dp < BL_MAX_DP; ++dp) {
          const int d = 16 * dp + r;
          if (dp < DP && d < D) {
            float vj = gld(xb[s] + j * D + d);
            if (sb[s] != nullptr) vj = vj * aj;
            gu[s][dp] += gld(gb[s] + (int64_t)p * D + d) * vj;
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int kp = 0; kp < BL_MAX_DP; ++kp)
#pragma unroll
        for (int dp = 0; dp < BL_MAX_DP; ++dp)
          if (kp < DP && dp < DP) acc[kp][dp] = mma(av[s][kp], gu[s][dp], acc[kp][dp]);
    if ((t - first) % BL_CHAIN_TILES == BL_CHAIN_TILES - 1 || t + 1 == last) {
#pragma unroll
      for (int kp = 0; kp < BL_MAX_DP; ++kp)
#pragma unroll
        for (int dp = 0; dp < BL_MAX_DP; ++dp) {
          tot[kp][dp] += acc[kp][dp];
          acc[kp][dp] = mf4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }

  // register c of lane (r, g) is gW[k = 16 kp + 4 g + c][d = 16 dp + r]
  float* pw = ws + ((int64_t)blockIdx.y * gridDim.x + q) * D * D;
#pragma unroll
  for (int kp = 0; kp < BL_MAX_DP; ++kp)
#pragma unroll
    for (int dp = 0; dp < BL_MAX_DP; ++dp)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 16 * kp + 4 * g + c, d = 16 * dp + r;
        if (kp < DP && dp < DP && k < D && d < D) gst(pw + k * D + d, tot[kp][dp][c]);
      }
}

// grad_W[o] = the partials of its `group` matrices over the slices (slices
// outer); n = elements of grad_W, Q = matrices of a slice.  A block takes 16
// elements; thread (e, y) adds the terms y, y + 16, ... in ascending order and
// thread (e, 0) the 16 sums in ascending y.
__global__ __launch_bounds__(256) void bilinear_finish_kernel(const float* __restrict__ ws,
                                                              int slices, int Q, int group, int DD,
                                                              int64_t n, float* __restrict__ gw) {
  __shared__ float part[16][17];
  const int ex = threadIdx.x & 15, y = threadIdx.x >> 4;
  const int64_t e = (int64_t)blockIdx.x * 16 + ex;
  float v = 0.0f;
  if (e < n) {
    const int64_t o = e / DD, w = e - o * DD;
    for (int t = y; t < slices * group; t += 16) {
      const int s = t / group, q = t - s * group;
      v += gld(ws + ((int64_t)s * Q + o * group + q) * DD + w);
    }
  }
  part[y][ex] = v;
  __syncthreads();
  if (y == 0 && e < n) {
    float sum = part[0][ex];
#pragma unroll
    for (int k = 1; k < 16; ++k) sum += part[k][ex];
    gst(gw + e, sum);
  }
}

bool bilinear_native(int kind, int64_t B, int64_t m, int64_t D) {
  return kind >= BL_ALL && kind <= BL_INTERACTION && B >= 1 && m >= 2 && m <= BL_MAX_M && D >= 1 &&
         D <= BL_MAX_D && B <= BL_MAX_B;
}

int bilinear_check(const char* what, int kind, int64_t B, int64_t m, int64_t D) {
  DR_REQUIRE(kind >= BL_ALL && kind <= BL_INTERACTION, DR_INVALID_ARGUMENT,
             "%s (bilinear): kind %d is not 0 (all), 1 (each) or 2 (interaction)", what, kind);
  DR_REQUIRE(m >= 2 && m <= BL_MAX_M, DR_INVALID_ARGUMENT,
             "%s (bilinear): fields %lld is outside [2, %d]", what, (long long)m, BL_MAX_M);
  DR_REQUIRE(D >= 1 && D <= BL_MAX_D, DR_INVALID_ARGUMENT,
             "%s (bilinear): embedding width %lld is outside [1, %d]", what, (long long)D,
             BL_MAX_D);
  DR_REQUIRE(B >= 1 && B <= BL_MAX_B, DR_INVALID_ARGUMENT,
             "%s (bilinear): batch %lld is outside [1, 2^31)", what, (long long)B);
  return DR_OK;
}

// LDS bytes of the staged tile, or 0 when the waves read global memory.
size_t tile_lds(int64_t m, int64_t D) {
  const size_t fl = (size_t)16 * tile_stride((int)m, (int)D);
  return fl <= (size_t)BL_LDS_FLOATS ? fl * sizeof(float) : 0;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" size_t dr_bilinear_workspace_size(int kind, int64_t B, int64_t m, int64_t D) {
  if (!bilinear_native(kind, B, m, D)) return 0;
  const WgPlan p = wg_plan(kind, B, m, D);
  return (size_t)p.slices * p.Q * D * D * sizeof(float);
}

extern "C" int dr_bilinear_forward(const float* x, const float* scale, const float* weight,
                                   int kind, int64_t B, int64_t m, int64_t D, float* out,
                                   void* stream) {
  const char* what = "dr_bilinear_forward";
  if (int rc = bilinear_check(what, kind, B, m, D)) return rc;
  DR_REQUIRE(x && weight && out, DR_INVALID_ARGUMENT, "%s (bilinear): a required pointer is null",
             what);
  const dim3 grid((unsigned)ceil_div(B, 16), (unsigned)ceil_div(m - 1, BL_WAVES));
  const size_t lds = tile_lds(m, D);
  if (lds)
    hipLaunchKernelGGL(bilinear_forward_kernel<true>, grid, dim3(BL_THREADS), lds, S(stream), x,
                       scale, weight, kind, B, (int)m, (int)D, out);
  else
    hipLaunchKernelGGL(bilinear_forward_kernel<false>, grid, dim3(BL_THREADS), 0, S(stream), x,
                       scale, weight, kind, B, (int)m, (int)D, out);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_bilinear_backward(const float* x, const float* scale, const float* weight,
                                    const float* grad_out, int kind, int64_t B, int64_t m,
                                    int64_t D, float* grad_x, float* grad_scale,
                                    float* grad_weight, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const char* what = "dr_bilinear_backward";
  if (int rc = bilinear_check(what, kind, B, m, D)) return rc;
  DR_REQUIRE(x && weight && grad_out && grad_x && grad_weight, DR_INVALID_ARGUMENT,
             "%s (bilinear): a required pointer is null", what);
  DR_REQUIRE(scale != nullptr || grad_scale == nullptr, DR_INVALID_ARGUMENT,
             "%s (bilinear): grad_scale without scale", what);
  const size_t need = dr_bilinear_workspace_size(kind, B, m, D);
  DR_REQUIRE(workspace != nullptr && workspace_bytes >= need, DR_INVALID_ARGUMENT,
             "%s (bilinear): workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  {
    const dim3 grid((unsigned)ceil_div(B, 16), (unsigned)ceil_div(m, BL_WAVES));
    const size_t lds = tile_lds(m, D);
    if (lds)
      hipLaunchKernelGGL(bilinear_input_grad_kernel<true>, grid, dim3(BL_THREADS), lds, S(stream),
                         x, scale, weight, grad_out, kind, B, (int)m, (int)D, grad_x, grad_scale);
    else
      hipLaunchKernelGGL(bilinear_input_grad_kernel<false>, grid, dim3(BL_THREADS), 0, S(stream),
                         x, scale, weight, grad_out, kind, B, (int)m, (int)D, grad_x, grad_scale);
    DR_LAUNCH_CHECK();
  }
  const WgPlan p = wg_plan(kind, B, m, D);
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(bilinear_weight_grad_kernel, dim3((unsigned)p.Q, (unsigned)p.slices),
                     dim3(64), 0, S(stream), x, scale, grad_out, kind, B, (int)m, (int)D, p.tiles,
                     ws);
  DR_LAUNCH_CHECK();
  const int64_t n = (kind == BL_ALL ? 1 : p.Q) * D * D;
  hipLaunchKernelGGL(bilinear_finish_kernel, dim3((unsigned)ceil_div(n, 16)), dim3(256), 0,
                     S(stream), ws, p.slices, p.Q, kind == BL_ALL ? p.Q : 1, (int)(D * D), n,
                     grad_weight);
  DR_LAUNCH_CHECK();
  return DR_OK;
}
