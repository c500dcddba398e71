// layer_norm.hip -- layer normalisation over the last axis with the pieces the
// models put around it fused in: a residual add in front, a relu and P
// elementwise masks behind; forward one launch, backward one launch plus a
// small finishing launch, fp32.
//
//   s    = x + residual                                   [B, D]
//   mean = mean_D(s)      var = mean_D((s - mean)^2)      rstd = 1 / sqrt(var + eps)
//   xhat = (s - mean) * rstd      u = gain * xhat + bias      a = relu ? max(u, 0) : u
//   out  = a                      [B, D]       without masks
//   out[:, p] = a * mask[:, p]    [B, P, D]    with them
//
//   da = sum_p dy_p * mask_p      dmask_p = dy_p * a      du = da * [u > 0]
//   dgain = sum_rows du * xhat    dbias = sum_rows du     dxhat = du * gain
//   ds = rstd * (dxhat - mean_D(dxhat) - xhat * mean_D(dxhat * xhat))
//
// About 1 flop per byte: VALU work bounded by HBM, no matrix instructions.  A
// row of D floats is Q = D / 4 float4 chunks.  A row owns G = next_pow2(Q)
// clipped to [1, 64] adjacent lanes of one wave (G = 1 << ll); lane c of them
// holds the chunks c, c + G, ..., C = ceil(Q / G) <= 4 of them, in registers
// (chunks at or past Q are absent and enter every sum as zeros).  A wave holds
// 64 / G rows and a block of 4 waves a tile of 256 / G rows.  G and C depend on
// D alone, so a row's results do not depend on B, on its place in the batch
// or on its neighbours.
//
// Forward: s is loaded once.  The lane sums its chunks in ascending order,
// the group's lanes are summed by the butterfly x += x(partner) at distances
// 1, 2, ..., G / 2 (DPP for the first four steps, the LDS crossbar for 16 and
// 32; every lane ends with the same bits), mean = sum / D.  The variance is a
// second pass over the registers from (s - mean), never E[s^2] - mean^2.
// Then u, a, and the P masks are streamed, each product stored as it is
// formed.  (mean, rstd) per row is the only saved tensor.  No LDS, no scratch.
//
// Backward: the grid is persistent, min(tiles, 1024) blocks, a function of
// (B, D) alone; block j visits the tiles j, j + grid, ...  Per row s is
// reloaded, xhat, u and a rebuilt with the forward's operations (the same
// bits), da formed over p ascending while dmask_p is stored, and the two row
// sums go through the butterfly together.  A lane's columns are the same in
// every tile, so it accumulates dgain / dbias for them in registers over the
// rows it visits, in ascending row order.  At the end of the block the lanes
// that hold the same columns in the wave's other rows are combined at
// distances G, 2 G, ..., 32, the four waves through LDS in wave order, and the
// block's [2, D] partial goes to the workspace.  The finishing kernel sums the
// partials of a column in a fixed order (sixteen interleaved runs over the
// blocks, each ascending, then the sixteen in order).  No atomics anywhere: two
// runs give the same bits and both directions capture into a graph.
#include <math.h>

#include "dr_common.h"

namespace dr {
namespace {

constexpr int LN_MAX_D = 1024, LN_MAX_P = 8;
constexpr int LN_THREADS = 256, LN_WAVES = LN_THREADS / 64;
constexpr int LN_MAX_BLOCKS = 1024;        // the persistent backward grid: 4 blocks per CU
constexpr int LN_FIN_COLS = 16, LN_FIN_RUNS = LN_THREADS / LN_FIN_COLS;

struct LnGeometry {
  int ll;                                  // log2 of the lanes per row
  int chunks;                              // float4 chunks per lane
  int tile;                                // rows per block
};

LnGeometry ln_geometry(int64_t D) {
  LnGeometry g;
  const int64_t Q = D / 4;
  g.ll = 0;
  while ((1 << g.ll) < Q && g.ll < 6) ++g.ll;
  g.chunks = (int)ceil_div(Q, (int64_t)1 << g.ll);
  g.tile = LN_THREADS >> g.ll;
  return g;
}

int64_t ln_tiles(int64_t B, const LnGeometry& g) { return ceil_div(B, g.tile); }
int64_t ln_blocks(int64_t B, const LnGeometry& g) {
  const int64_t t = ln_tiles(B, g);
  return t < LN_MAX_BLOCKS ? t : LN_MAX_BLOCKS;
}

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// Sum over the 1 << ll adjacent lanes of a row; all of them get the same bits.
// Steps 1 and 2 are the quad permutes lane ^ 1 and lane ^ 2; a quad then holds
// one value, so the mirrors of 8 and of 16 lanes add the same pairs as lane ^ 4
// and lane ^ 8 would.  Every lane of the wave must be here.
__device__ __forceinline__ float group_sum(float x, int ll) {
  if (ll > 0) x += dpp<0xB1>(x);           // quad_perm:[1,0,3,2]
  if (ll > 1) x += dpp<0x4E>(x);           // quad_perm:[2,3,0,1]
  if (ll > 2) x += dpp<0x141>(x);          // row_half_mirror
  if (ll > 3) x += dpp<0x140>(x);          // row_mirror
  if (ll > 4) x += __shfl_xor(x, 16, 64);
  if (ll > 5) x += __shfl_xor(x, 32, 64);
  return x;
}

// Sum over the lanes that hold the same chunk in the other rows of the wave.
__device__ __forceinline__ float column_sum(float x, int ll) {
  for (int d = 1 << ll; d < 64; d <<= 1) x += __shfl_xor(x, d, 64);
  return x;
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float sum4(float4 v, float acc) {
  return (((acc + v.x) + v.y) + v.z) + v.w;
}
__device__ __forceinline__ float dot4(float4 a, float4 b, float p) {
  p = fmaf(a.x, b.x, p);
  p = fmaf(a.y, b.y, p);
  p = fmaf(a.z, b.z, p);
  return fmaf(a.w, b.w, p);
}
__device__ __forceinline__ float4 ld4(const float* p) {
  return gld(reinterpret_cast<const float4*>(p));
}
__device__ __forceinline__ void st4(float* p, float4 v) { gst(reinterpret_cast<float4*>(p), v); }

#define LN_EACH(EXPR_X, EXPR_Y, EXPR_Z, EXPR_W) make_float4(EXPR_X, EXPR_Y, EXPR_Z, EXPR_W)

// The thread's place in the block's tile and the columns it holds.
template <int C>
struct LnLane {
  int r, c;                                // row of the tile, lane of the row
  int col[C];                              // first column of chunk i
  bool has[C];                             // chunk i lies inside the row
  __device__ LnLane(int ll, int D) {
    const int lane = threadIdx.x & 63;
    r = (int)(threadIdx.x >> 6) * (64 >> ll) + (lane >> ll);
    c = lane & ((1 << ll) - 1);
#pragma unroll
    for (int i = 0; i < C; ++i) {
      col[i] = 4 * (c + (i << ll));
      has[i] = col[i] < D;
    }
  }
};

// xhat, u and a of one chunk from (s - mean); the forward and the backward
// both go through here, so the backward rebuilds the forward's bits.
struct LnPoint {
  float4 xh, u, a;
};
__device__ __forceinline__ LnPoint ln_point(float4 d, float rstd, float4 g, float4 b, bool relu) {
  LnPoint p;
  p.xh = LN_EACH(d.x * rstd, d.y * rstd, d.z * rstd, d.w * rstd);
  p.u = LN_EACH(g.x * p.xh.x + b.x, g.y * p.xh.y + b.y, g.z * p.xh.z + b.z, g.w * p.xh.w + b.w);
  p.a = p.u;
  if (relu)
    p.a = LN_EACH(p.u.x < 0.f ? 0.f : p.u.x, p.u.y < 0.f ? 0.f : p.u.y, p.u.z < 0.f ? 0.f : p.u.z,
                  p.u.w < 0.f ? 0.f : p.u.w);
  return p;
}

template <int C>
__global__ __launch_bounds__(LN_THREADS) void layer_norm_forward_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ res, int64_t ld_res,
    const float* __restrict__ gain, const float* __restrict__ bias,
    const float* __restrict__ mask, int64_t ld_mask, int64_t B, int D, int P, int ll, float eps,
    int relu, float* __restrict__ out, float* __restrict__ saved) {
  const LnLane<C> at(ll, D);
  const int64_t row = (int64_t)blockIdx.x * (LN_THREADS >> ll) + at.r;
  const bool live = row < B;               // idle lanes stay for the butterflies, with zeros
  const int64_t rb = live ? row : 0;       // (and form no address they use)
  const float fd = (float)D;

  float4 s[C], g[C], b[C];
  bool on[C];
  float sum = 0.0f;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    on[i] = live && at.has[i];
    g[i] = at.has[i] ? ld4(gain + at.col[i]) : zero4();
    b[i] = at.has[i] ? ld4(bias + at.col[i]) : zero4();
    s[i] = on[i] ? ld4(x + rb * ld_x + at.col[i]) : zero4();
    if (res != nullptr && on[i]) {
      const float4 t = ld4(res + rb * ld_res + at.col[i]);
      s[i] = LN_EACH(s[i].x + t.x, s[i].y + t.y, s[i].z + t.z, s[i].w + t.w);
    }
    sum = sum4(s[i], sum);
  }
  const float mean = group_sum(sum, ll) / fd;
  float sq = 0.0f;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    s[i] = on[i] ? LN_EACH(s[i].x - mean, s[i].y - mean, s[i].z - mean, s[i].w - mean) : zero4();
    sq = dot4(s[i], s[i], sq);
  }
  const float rstd = 1.0f / sqrtf(group_sum(sq, ll) / fd + eps);
  if (live && at.c == 0) {
    gst(saved + 2 * row, mean);
    gst(saved + 2 * row + 1, rstd);
  }

  float4 a[C];
#pragma unroll
  for (int i = 0; i < C; ++i) a[i] = ln_point(s[i], rstd, g[i], b[i], relu != 0).a;
  if (mask == nullptr) {
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (on[i]) st4(out + rb * D + at.col[i], a[i]);
    return;
  }
  const float* mr = mask + rb * ld_mask;
  float* orow = out + rb * (int64_t)P * D;
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (on[i]) {
        const float4 m = ld4(mr + p * D + at.col[i]);
        st4(orow + p * D + at.col[i], LN_EACH(a[i].x * m.x, a[i].y * m.y, a[i].z * m.z, a[i].w * m.w));
      }
  }
}

template <int C>
__global__ __launch_bounds__(LN_THREADS) void layer_norm_backward_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ res, int64_t ld_res,
    const float* __restrict__ gain, const float* __restrict__ bias,
    const float* __restrict__ mask, int64_t ld_mask, const float* __restrict__ saved,
    const float* __restrict__ dy, int64_t ld_dy, int64_t B, int D, int P, int ll, int relu,
    int64_t tiles, float* __restrict__ dx, float* __restrict__ dmask, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) float part[];   // [waves][2][D]
  const LnLane<C> at(ll, D);
  const int tile = LN_THREADS >> ll;
  const float fd = (float)D;

  float4 g[C], b[C], ag[C], ab[C];
#pragma unroll
  for (int i = 0; i < C; ++i) {
    g[i] = at.has[i] ? ld4(gain + at.col[i]) : zero4();
    b[i] = at.has[i] ? ld4(bias + at.col[i]) : zero4();
    ag[i] = ab[i] = zero4();
  }

  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // (uniform over the block)
    const int64_t row = t * tile + at.r;
    const bool live = row < B;
    const int64_t rb = live ? row : 0;
    const float mean = live ? gld(saved + 2 * rb) : 0.0f;
    const float rstd = live ? gld(saved + 2 * rb + 1) : 0.0f;
    bool on[C];
    LnPoint pt[C];
    float4 da[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
      on[i] = live && at.has[i];
      float4 s = on[i] ? ld4(x + rb * ld_x + at.col[i]) : zero4();
      if (res != nullptr && on[i]) {
        const float4 r = ld4(res + rb * ld_res + at.col[i]);
        s = LN_EACH(s.x + r.x, s.y + r.y, s.z + r.z, s.w + r.w);
      }
      s = on[i] ? LN_EACH(s.x - mean, s.y - mean, s.z - mean, s.w - mean) : zero4();
      pt[i] = ln_point(s, rstd, g[i], b[i], relu != 0);
      da[i] = zero4();
    }
    const float* gr = dy + rb * ld_dy;
    if (mask == nullptr) {
#pragma unroll
      for (int i = 0; i < C; ++i)
        if (on[i]) da[i] = ld4(gr + at.col[i]);
    } else {
      const float* mr = mask + rb * ld_mask;
      float* dm = dmask + rb * (int64_t)P * D;
      for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int i = 0; i < C; ++i)
          if (on[i]) {
            const float4 v = ld4(gr + p * D + at.col[i]);
            const float4 m = ld4(mr + p * D + at.col[i]);
            const float4 a = pt[i].a;
            st4(dm + p * D + at.col[i], LN_EACH(v.x * a.x, v.y * a.y, v.z * a.z, v.w * a.w));
            da[i] = LN_EACH(fmaf(v.x, m.x, da[i].x), fmaf(v.y, m.y, da[i].y),
                            fmaf(v.z, m.z, da[i].z), fmaf(v.w, m.w, da[i].w));
          }
      }
    }
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const float4 u = pt[i].u, xh = pt[i].xh;
      float4 du = da[i];
      if (relu)
        du = LN_EACH(u.x > 0.f ? du.x : 0.f, u.y > 0.f ? du.y : 0.f, u.z > 0.f ? du.z : 0.f,
                     u.w > 0.f ? du.w : 0.f);
      ag[i] = LN_EACH(ag[i].x + du.x * xh.x, ag[i].y + du.y * xh.y, ag[i].z + du.z * xh.z,
                      ag[i].w + du.w * xh.w);
      ab[i] = LN_EACH(ab[i].x + du.x, ab[i].y + du.y, ab[i].z + du.z, ab[i].w + du.w);
      da[i] = LN_EACH(du.x * g[i].x, du.y * g[i].y, du.z * g[i].z, du.w * g[i].w);   // dxhat
      s1 = sum4(da[i], s1);
      s2 = dot4(da[i], xh, s2);
    }
    const float m1 = group_sum(s1, ll) / fd, m2 = group_sum(s2, ll) / fd;
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (on[i]) {
        const float4 d = da[i], xh = pt[i].xh;
        st4(dx + rb * D + at.col[i],
            LN_EACH(rstd * ((d.x - m1) - xh.x * m2), rstd * ((d.y - m1) - xh.y * m2),
                    rstd * ((d.z - m1) - xh.z * m2), rstd * ((d.w - m1) - xh.w * m2)));
      }
  }

  // the block's column sums: the wave's rows, then the waves in order
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    if (C == 1) {                          // (C > 1 has one row per wave)
      ag[i] = LN_EACH(column_sum(ag[i].x, ll), column_sum(ag[i].y, ll), column_sum(ag[i].z, ll),
                      column_sum(ag[i].w, ll));
      ab[i] = LN_EACH(column_sum(ab[i].x, ll), column_sum(ab[i].y, ll), column_sum(ab[i].z, ll),
                      column_sum(ab[i].w, ll));
    }
    if (((threadIdx.x & 63) >> ll) == 0 && at.has[i]) {
      *reinterpret_cast<float4*>(part + (wave * 2 + 0) * D + at.col[i]) = ag[i];
      *reinterpret_cast<float4*>(part + (wave * 2 + 1) * D + at.col[i]) = ab[i];
    }
  }
  __syncthreads();
  float* wb = ws + (int64_t)blockIdx.x * 2 * D;
  for (int j = threadIdx.x; j < 2 * D; j += LN_THREADS) {
    float v = part[j];
#pragma unroll
    for (int w = 1; w < LN_WAVES; ++w) v += part[w * 2 * D + j];
    gst(wb + j, v);
  }
}

// dgain | dbias [2 D] from the blocks' partials [blocks, 2 D]: a block of the
// grid takes 16 columns, run r of its 16 the blocks r, r + 16, ... ascending
// (independent loads, eight in flight per lane; 1024 partials are 64 a run).
__global__ __launch_bounds__(LN_THREADS) void layer_norm_finish_kernel(
    const float* __restrict__ ws, int blocks, int D, float* __restrict__ dgain,
    float* __restrict__ dbias) {
  __shared__ float runs[LN_FIN_RUNS][LN_FIN_COLS];
  const int jl = threadIdx.x % LN_FIN_COLS, r = threadIdx.x / LN_FIN_COLS;
  const int j = blockIdx.x * LN_FIN_COLS + jl;
  float v = 0.0f;
  if (j < 2 * D)
#pragma unroll 8
    for (int k = r; k < blocks; k += LN_FIN_RUNS) v += gld(ws + (int64_t)k * 2 * D + j);
  runs[r][jl] = v;
  __syncthreads();
  if (r == 0 && j < 2 * D) {
    v = runs[0][jl];
#pragma unroll
    for (int k = 1; k < LN_FIN_RUNS; ++k) v += runs[k][jl];
    gst(j < D ? dgain + j : dbias + (j - D), v);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int ln_check(const char* what, int64_t B, int64_t D, int64_t P, const void* mask) {
  DR_REQUIRE(D >= 4 && D <= LN_MAX_D && D % 4 == 0, DR_INVALID_ARGUMENT,
             "%s (layer_norm): width %lld is not a multiple of 4 in [4, %d]", what, (long long)D,
             LN_MAX_D);
  DR_REQUIRE(P >= 1 && P <= LN_MAX_P, DR_INVALID_ARGUMENT,
             "%s (layer_norm): masks %lld is outside [1, %d]", what, (long long)P, LN_MAX_P);
  DR_REQUIRE(mask != nullptr || P == 1, DR_INVALID_ARGUMENT,
             "%s (layer_norm): masks %lld without a mask tensor", what, (long long)P);
  DR_REQUIRE(B >= 0 && B <= (int64_t(1) << 31) - 1, DR_INVALID_ARGUMENT,
             "%s (layer_norm): batch %lld is outside [0, 2^31)", what, (long long)B);
  return DR_OK;
}

int ln_rows(const char* what, const char* name, const void* p, bool required, int64_t ld,
            int64_t least) {
  if (p == nullptr && !required) return DR_OK;
  DR_REQUIRE(p != nullptr && aligned16(p), DR_INVALID_ARGUMENT,
             "%s (layer_norm): %s is null or not 16-byte aligned", what, name);
  DR_REQUIRE(ld >= least && ld % 4 == 0, DR_INVALID_ARGUMENT,
             "%s (layer_norm): the row stride of %s = %lld is below %lld or not a multiple of 4 "
             "floats", what, name, (long long)ld, (long long)least);
  return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

#define DR_LN_DISPATCH(LAUNCH)   \
  switch (g.chunks) {            \
    case 1: LAUNCH(1); break;    \
    case 2: LAUNCH(2); break;    \
    case 3: LAUNCH(3); break;    \
    default: LAUNCH(4); break;   \
  }

extern "C" size_t dr_layer_norm_saved_size(int64_t B) {
  return B <= 0 ? 0 : (size_t)B * 2 * sizeof(float);
}

extern "C" size_t dr_layer_norm_workspace_size(int64_t B, int64_t D) {
  if (B <= 0 || D < 4 || D > LN_MAX_D || D % 4) return 0;
  return (size_t)ln_blocks(B, ln_geometry(D)) * 2 * (size_t)D * sizeof(float);
}

extern "C" int dr_layer_norm_forward(const float* x, int64_t ld_x, const float* residual,
                                     int64_t ld_residual, const float* gain, const float* bias,
                                     const float* mask, int64_t ld_mask, int64_t B, int64_t D,
                                     int64_t P, float eps, int relu, float* out, float* saved,
                                     void* stream) {
  const char* what = "dr_layer_norm_forward";
  if (int rc = ln_check(what, B, D, P, mask)) return rc;
  if (int rc = ln_rows(what, "x", x, true, ld_x, D)) return rc;
  if (int rc = ln_rows(what, "residual", residual, false, ld_residual, D)) return rc;
  if (int rc = ln_rows(what, "mask", mask, false, ld_mask, P * D)) return rc;
  DR_REQUIRE(gain && bias && out && saved && aligned16(gain) && aligned16(bias) &&
                 aligned16(out) && aligned16(saved),
             DR_INVALID_ARGUMENT,
             "%s (layer_norm): gain, bias, out or saved is null or not 16-byte aligned", what);
  DR_REQUIRE(eps >= 0.0f, DR_INVALID_ARGUMENT, "%s (layer_norm): eps %g is negative", what,
             (double)eps);
  if (B == 0) return DR_OK;
  const LnGeometry g = ln_geometry(D);
  const dim3 grid((unsigned)ln_tiles(B, g)), block(LN_THREADS);
#define DR_LN_FWD(CC)                                                                          \
  hipLaunchKernelGGL((layer_norm_forward_kernel<CC>), grid, block, 0, S(stream), x, ld_x,      \
                     residual, ld_residual, gain, bias, mask, ld_mask, B, (int)D, (int)P, g.ll, \
                     eps, relu, out, saved)
  DR_LN_DISPATCH(DR_LN_FWD)
#undef DR_LN_FWD
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_layer_norm_backward(const float* x, int64_t ld_x, const float* residual,
                                      int64_t ld_residual, const float* gain, const float* bias,
                                      const float* mask, int64_t ld_mask, const float* saved,
                                      const float* grad_out, int64_t ld_grad_out, int64_t B,
                                      int64_t D, int64_t P, int relu, float* grad_x,
                                      float* grad_mask, float* grad_gain, float* grad_bias,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "dr_layer_norm_backward";
  if (int rc = ln_check(what, B, D, P, mask)) return rc;
  if (int rc = ln_rows(what, "x", x, true, ld_x, D)) return rc;
  if (int rc = ln_rows(what, "residual", residual, false, ld_residual, D)) return rc;
  if (int rc = ln_rows(what, "mask", mask, false, ld_mask, P * D)) return rc;
  if (int rc = ln_rows(what, "grad_out", grad_out, true, ld_grad_out, P * D)) return rc;
  DR_REQUIRE(gain && bias && saved && grad_x && grad_gain && grad_bias && aligned16(gain) &&
                 aligned16(bias) && aligned16(saved) && aligned16(grad_x) &&
                 aligned16(grad_gain) && aligned16(grad_bias),
             DR_INVALID_ARGUMENT,
             "%s (layer_norm): gain, bias, saved or a gradient is null or not 16-byte aligned",
             what);
  DR_REQUIRE((mask == nullptr) == (grad_mask == nullptr) && aligned16(grad_mask),
             DR_INVALID_ARGUMENT,
             "%s (layer_norm): grad_mask must be given with mask, 16-byte aligned", what);
  const size_t need = dr_layer_norm_workspace_size(B, D);
  DR_REQUIRE(workspace_bytes >= need && (need == 0 || (workspace && aligned16(workspace))),
             DR_INVALID_ARGUMENT,
             "%s (layer_norm): workspace of %zu bytes, %zu needed (16-byte aligned)", what,
             workspace_bytes, need);
  const LnGeometry g = ln_geometry(D);
  const int64_t tiles = ln_tiles(B, g), blocks = ln_blocks(B, g);
  float* ws = static_cast<float*>(workspace);
  if (B > 0) {
    const dim3 grid((unsigned)blocks), block(LN_THREADS);
    const size_t lds = (size_t)LN_WAVES * 2 * (size_t)D * sizeof(float);
#define DR_LN_BWD(CC)                                                                           \
  hipLaunchKernelGGL((layer_norm_backward_kernel<CC>), grid, block, lds, S(stream), x, ld_x,    \
                     residual, ld_residual, gain, bias, mask, ld_mask, saved, grad_out,         \
                     ld_grad_out, B, (int)D, (int)P, g.ll, relu, tiles, grad_x, grad_mask, ws)
    DR_LN_DISPATCH(DR_LN_BWD)
#undef DR_LN_BWD
    DR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(layer_norm_finish_kernel, dim3((unsigned)ceil_div(2 * D, LN_FIN_COLS)),
                     dim3(LN_THREADS), 0, S(stream), ws, (int)blocks, (int)D, grad_gain,
                     grad_bias);
  DR_LAUNCH_CHECK();
  return DR_OK;
}
