// gate_mix.hip -- the multi-gate mixture-of-experts block of MMoE / PLE: per
// (sample, task) a softmax gate over the experts the task may see, and the
// gate-weighted mixtures of the expert outputs; forward and backward, one
// launch each, fp32.
//
//   g[b,k,e]   = softmax over e in S_k of z[b,k,e]        (exactly 0 outside S_k)
//   out[b,k,:] = sum_e g[b,k,e] h[b,e,:]
//   dh[b,e,:]  = sum_k g[b,k,e] go[b,k,:]     dg[b,k,e] = dot(go[b,k,:], h[b,e,:])
//   dz[b,k,e]  = g[b,k,e] (dg[b,k,e] - sum_e' g[b,k,e'] dg[b,k,e'])   (0 outside S_k)
//
// This is VALU work bounded by HBM (about 1 flop per byte): no matrix
// instructions.  A row of H floats is Q = H / 4 float4 chunks.  A sample owns
// LPS = max(4, next_pow2(min(Q, 64))) adjacent lanes of one wave, lane c of
// them the chunk c (and the chunk c + 64 when Q > 64; lanes with c >= Q only
// take part in the reductions, with zeros), so a wave holds 64 / LPS samples
// and a block of W waves a tile of W * 64 / LPS samples.  W is 4, halved while
// the tile's gates would need more than 32 KB of LDS.  LPS depends on H alone
// and W never enters a sum, so a sample's results do not depend on B, on its
// place in the batch or on its neighbours.
//
// Forward: the block's threads take the tile's (sample, task) rows, one lane
// per row: max, then exp and sum, then the quotients, each over e ascending,
// through the tile's gates in LDS (row stride K E | 1: the samples of a wave
// read different banks).  After one barrier gates[] is written from LDS in
// coalesced order and the column lanes stream h once: for e ascending they
// load the chunk of expert e and, for every task, acc_k = fma(g[k,e], h, acc_k)
// with g broadcast from LDS; the K accumulators stay in registers.  Unselected
// experts enter with their exact-zero gate.
//
// Backward: the tile's gates go to LDS; a lane keeps its K grad_out chunks in
// registers and, for e ascending, loads the chunk of expert e once, stores
// dh = fma(g[k,e], go_k, dh) over k ascending from 0, and forms its K partial
// dot products p = fma(go_k[j], h[j], p) over its columns j ascending (chunk c,
// then chunk c + 64) from 0.  The partials are summed over the sample's lanes
// by the butterfly x += x(partner), partners at distance 1, 2, ..., LPS / 2
// (group_sum: pairs, quads, eights, ... in that order): every lane ends with
// the same bits, and lane 0 puts dg[k,e] in LDS.  After one barrier the
// lane that owns a gate row forms dot = fma(g[e], dg[e], dot) over the selected
// e ascending from 0 and dz[e] = g[e] * (dg[e] - dot).  A row with one selected
// expert has g = 1, dot = dg and dz = 0 exactly.  No atomics, no scratch.
#include <math.h>

#include "dr_common.h"

namespace dr {
namespace {

constexpr int GM_MAX_K = 8, GM_MAX_E = 16, GM_MAX_H = 512;
constexpr int GM_WAVES = 4;
constexpr int GM_LDS_BYTES = 32 << 10;     // the backward's two [tile, K E | 1] arrays

struct GmSelect {                          // S_k as bits, by value: a captured launch keeps it
  uint32_t w[GM_MAX_K];
};

struct GmGeometry {
  int ll;                                  // log2 of the lanes per sample
  int waves;                               // waves per block
  int tile;                                // samples per block
  size_t lds;                              // bytes of one [tile, K E | 1] array
};

GmGeometry gm_geometry(int64_t K, int64_t E, int64_t H) {
  GmGeometry g;
  const int64_t Q = H / 4;
  g.ll = 2;
  while ((1 << g.ll) < Q && g.ll < 6) ++g.ll;
  const int spw = 64 >> g.ll;
  const size_t row = (size_t)((K * E) | 1) * sizeof(float);
  g.waves = GM_WAVES;
  while (g.waves > 1 && 2 * g.waves * spw * row > (size_t)GM_LDS_BYTES) g.waves >>= 1;
  g.tile = g.waves * spw;
  g.lds = g.tile * row;
  return g;
}

template <int K>
__device__ __forceinline__ uint32_t select_of(const GmSelect& sel, int k) {
  uint32_t bits = 0;                       // (no per-lane index into the argument struct)
#pragma unroll
  for (int kk = 0; kk < K; ++kk) bits = k == kk ? sel.w[kk] : bits;
  return bits;
}

__device__ __forceinline__ float4 fma4(float a, float4 x, float4 c) {
  return make_float4(fmaf(a, x.x, c.x), fmaf(a, x.y, c.y), fmaf(a, x.z, c.z), fmaf(a, x.w, c.w));
}
__device__ __forceinline__ float dot4(float4 a, float4 b, float p) {
  p = fmaf(a.x, b.x, p);
  p = fmaf(a.y, b.y, p);
  p = fmaf(a.z, b.z, p);
  return fmaf(a.w, b.w, p);
}

template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// Sum over the 1 << ll (>= 4) adjacent lanes of a sample; all lanes get the
// same bits.  Steps 1 and 2 are the quad permutes lane ^ 1 and lane ^ 2; a
// quad then holds one value, so the mirrors of 8 and of 16 lanes add the same
// pairs as lane ^ 4 and lane ^ 8 would.  All four are DPP operands, off the
// LDS pipe; the steps of 16 and 32 go through it.
__device__ __forceinline__ float group_sum(float x, int ll) {
  x += dpp<0xB1>(x);                       // quad_perm:[1,0,3,2]
  x += dpp<0x4E>(x);                       // quad_perm:[2,3,0,1]
  if (ll > 2) x += dpp<0x141>(x);          // row_half_mirror
  if (ll > 3) x += dpp<0x140>(x);          // row_mirror
  if (ll > 4) x += __shfl_xor(x, 16, 64);
  if (ll > 5) x += __shfl_xor(x, 32, 64);
  return x;
}

// The thread's place among the column lanes of the block's tile.
struct GmLane {
  int sl, c;                               // sample of the tile, chunk lane of the sample
  __device__ GmLane(int ll) {
    const int lane = threadIdx.x & 63;
    sl = (int)(threadIdx.x >> 6) * (64 >> ll) + (lane >> ll);
    c = lane & ((1 << ll) - 1);
  }
};

template <int K, int CPL>
__global__ __launch_bounds__(GM_WAVES * 64) void gate_mix_forward_kernel(
    const float* __restrict__ z, int64_t ld_z, const float* __restrict__ h, int64_t ld_h,
    GmSelect sel, int64_t B, int E, int H, int ll, float* __restrict__ out,
    float* __restrict__ gates) {
  extern __shared__ __attribute__((aligned(16))) float sg[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int KE = K * E, gs = KE | 1;
  const int tile = (nthr >> 6) * (64 >> ll);
  const int64_t b0 = (int64_t)blockIdx.x * tile;
  const int nb = B - b0 < tile ? (int)(B - b0) : tile;

  for (int r = tid; r < nb * K; r += nthr) {               // one lane per gate row
    const int sl = r / K, k = r - sl * K;
    const uint32_t bits = select_of<K>(sel, k);
    const float* zr = z + (b0 + sl) * ld_z + k * E;
    float* gr = sg + sl * gs + k * E;
    float m = -INFINITY;
    for (int e = 0; e < E; ++e)
      if ((bits >> e) & 1) m = fmaxf(m, gld(zr + e));
    float s = 0.0f;
    for (int e = 0; e < E; ++e) {
      const float x = (bits >> e) & 1 ? expf(gld(zr + e) - m) : 0.0f;
      gr[e] = x;
      s += x;
    }
    for (int e = 0; e < E; ++e) gr[e] = gr[e] / s;
  }
  __syncthreads();

  float* gt = gates + b0 * KE;
  for (int i = tid; i < nb * KE; i += nthr) {
    const int sl = i / KE;
    gst(gt + i, sg[sl * gs + (i - sl * KE)]);
  }

  const GmLane at(ll);
  const int Q = H >> 2;
  if (at.sl >= nb || at.c >= Q) return;                    // (no barrier and no shuffle below)
  const float* gr = sg + at.sl * gs;
  const float* hb = h + (b0 + at.sl) * ld_h + 4 * at.c;
  float* ob = out + (b0 + at.sl) * (int64_t)K * H + 4 * at.c;
  const bool second = CPL > 1 && at.c + 64 < Q;
  float4 acc[K][CPL];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < CPL; ++i) acc[k][i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int e = 0; e < E; ++e) {
    float4 x[CPL];
    x[0] = gld(reinterpret_cast<const float4*>(hb + e * H));
    if constexpr (CPL > 1)
      x[1] = second ? gld(reinterpret_cast<const float4*>(hb + e * H + 256))
                    : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float g = gr[k * E + e];
#pragma unroll
      for (int i = 0; i < CPL; ++i) acc[k][i] = fma4(g, x[i], acc[k][i]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    gst(reinterpret_cast<float4*>(ob + k * H), acc[k][0]);
    if constexpr (CPL > 1)
      if (second) gst(reinterpret_cast<float4*>(ob + k * H + 256), acc[k][1]);
  }
}

template <int K, int CPL>
__global__ __launch_bounds__(GM_WAVES * 64) void gate_mix_backward_kernel(
    const float* __restrict__ h, int64_t ld_h, const float* __restrict__ gates,
    const float* __restrict__ go, int64_t ld_go, GmSelect sel, int64_t B, int E, int H, int ll,
    float* __restrict__ grad_z, float* __restrict__ grad_h) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int KE = K * E, gs = KE | 1;
  const int tile = (nthr >> 6) * (64 >> ll);
  const int64_t b0 = (int64_t)blockIdx.x * tile;
  const int nb = B - b0 < tile ? (int)(B - b0) : tile;
  float* sg = lds;                                         // the tile's gates
  float* sd = lds + tile * gs;                             // the tile's dg

  const float* gt = gates + b0 * KE;
  for (int i = tid; i < nb * KE; i += nthr) {
    const int sl = i / KE;
    sg[sl * gs + (i - sl * KE)] = gld(gt + i);
  }
  __syncthreads();

  // every lane of a wave stays for the butterflies; the idle ones carry zeros
  const GmLane at(ll);
  const int Q = H >> 2;
  const bool live = at.sl < nb;
  const bool on[2] = {live && at.c < Q, CPL > 1 && live && at.c + 64 < Q};
  const int64_t b = live ? b0 + at.sl : b0;                // (idle lanes form no address they use)
  const float* gr = sg + (live ? at.sl : 0) * gs;
  const float* hb = h + b * ld_h + 4 * at.c;
  const float* gb = go + b * ld_go + 4 * at.c;
  float* db = grad_h + b * (int64_t)E * H + 4 * at.c;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gk[K][CPL];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < CPL; ++i)
      gk[k][i] = on[i] ? gld(reinterpret_cast<const float4*>(gb + k * H + 256 * i)) : zero;
  for (int e = 0; e < E; ++e) {
    float4 x[CPL], d[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      x[i] = on[i] ? gld(reinterpret_cast<const float4*>(hb + e * H + 256 * i)) : zero;
      d[i] = zero;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float g = gr[k * E + e];
#pragma unroll
      for (int i = 0; i < CPL; ++i) d[i] = fma4(g, gk[k][i], d[i]);
    }
#pragma unroll
    for (int i = 0; i < CPL; ++i)
      if (on[i]) gst(reinterpret_cast<float4*>(db + e * H + 256 * i), d[i]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float p = 0.0f;
#pragma unroll
      for (int i = 0; i < CPL; ++i) p = dot4(gk[k][i], x[i], p);
      p = group_sum(p, ll);
      if (live && at.c == 0) sd[at.sl * gs + k * E + e] = p;
    }
  }
  __syncthreads();

  for (int r = tid; r < nb * K; r += nthr) {               // the lane that owns the gate row
    const int sl = r / K, k = r - sl * K;
    const uint32_t bits = select_of<K>(sel, k);
    const float* g = sg + sl * gs + k * E;
    const float* dg = sd + sl * gs + k * E;
    float* gz = grad_z + (b0 + sl) * KE + k * E;
    float dot = 0.0f;
    for (int e = 0; e < E; ++e)
      if ((bits >> e) & 1) dot = fmaf(g[e], dg[e], dot);
    for (int e = 0; e < E; ++e) gst(gz + e, (bits >> e) & 1 ? g[e] * (dg[e] - dot) : 0.0f);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int gm_check(const char* what, int64_t B, int64_t K, int64_t E, int64_t H,
             const uint32_t* select_bits, GmSelect& sel) {
  DR_REQUIRE(K >= 1 && K <= GM_MAX_K, DR_INVALID_ARGUMENT,
             "%s (gate_mix): tasks %lld is outside [1, %d]", what, (long long)K, GM_MAX_K);
  DR_REQUIRE(E >= 1 && E <= GM_MAX_E, DR_INVALID_ARGUMENT,
             "%s (gate_mix): experts %lld is outside [1, %d]", what, (long long)E, GM_MAX_E);
  DR_REQUIRE(H >= 4 && H <= GM_MAX_H && H % 4 == 0, DR_INVALID_ARGUMENT,
             "%s (gate_mix): width %lld is not a multiple of 4 in [4, %d]", what, (long long)H,
             GM_MAX_H);
  DR_REQUIRE(B >= 0 && B <= (int64_t(1) << 31) - 1, DR_INVALID_ARGUMENT,
             "%s (gate_mix): batch %lld is outside [0, 2^31)", what, (long long)B);
  const uint32_t all = (uint32_t)((1u << E) - 1u);
  for (int k = 0; k < GM_MAX_K; ++k) {
    sel.w[k] = k < K ? (select_bits ? select_bits[k] : all) : 0u;
    DR_REQUIRE(k >= K || (sel.w[k] != 0 && (sel.w[k] & ~all) == 0), DR_INVALID_ARGUMENT,
               "%s (gate_mix): selection word %d = 0x%x is empty or has a bit at or above %lld",
               what, k, sel.w[k], (long long)E);
  }
  return DR_OK;
}

int gm_stride(const char* what, const char* name, int64_t ld, int64_t least) {
  DR_REQUIRE(ld >= least && ld % 4 == 0, DR_INVALID_ARGUMENT,
             "%s (gate_mix): row stride %s = %lld is below %lld or not a multiple of 4 floats",
             what, name, (long long)ld, (long long)least);
  return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

// one case per K; the second chunk per lane only above 64 chunks
#define DR_GM_DISPATCH(LAUNCH)                 \
  switch (K) {                                 \
    case 1: LAUNCH(1); break;                  \
    case 2: LAUNCH(2); break;                  \
    case 3: LAUNCH(3); break;                  \
    case 4: LAUNCH(4); break;                  \
    case 5: LAUNCH(5); break;                  \
    case 6: LAUNCH(6); break;                  \
    case 7: LAUNCH(7); break;                  \
    default: LAUNCH(8); break;                 \
  }

extern "C" size_t dr_gate_mix_saved_size(int64_t B, int64_t K, int64_t E) {
  if (B <= 0 || K <= 0 || E <= 0) return 0;
  return (size_t)B * (size_t)K * (size_t)E * sizeof(float);
}

extern "C" int dr_gate_mix_forward(const float* z, int64_t ld_z, const float* h, int64_t ld_h,
                                   const uint32_t* select_bits, int64_t B, int64_t K, int64_t E,
                                   int64_t H, float* out, float* gates, void* stream) {
  const char* what = "dr_gate_mix_forward";
  GmSelect sel;
  if (int rc = gm_check(what, B, K, E, H, select_bits, sel)) return rc;
  if (int rc = gm_stride(what, "ld_z", ld_z, K * E)) return rc;
  if (int rc = gm_stride(what, "ld_h", ld_h, E * H)) return rc;
  DR_REQUIRE(z && h && out && gates, DR_INVALID_ARGUMENT,
             "%s (gate_mix): a required pointer is null", what);
  DR_REQUIRE(aligned16(z) && aligned16(h) && aligned16(out) && aligned16(gates),
             DR_INVALID_ARGUMENT, "%s (gate_mix): z, h, out and gates must be 16-byte aligned",
             what);
  if (B == 0) return DR_OK;
  const GmGeometry g = gm_geometry(K, E, H);
  const dim3 grid((unsigned)ceil_div(B, g.tile)), block(g.waves * 64);
#define DR_GM_FWD2(KK, CPL)                                                                     \
  hipLaunchKernelGGL((gate_mix_forward_kernel<KK, CPL>), grid, block, g.lds, S(stream), z, ld_z, \
                     h, ld_h, sel, B, (int)E, (int)H, g.ll, out, gates)
#define DR_GM_FWD(KK)                 \
  do {                                \
    if (H > 256) DR_GM_FWD2(KK, 2);   \
    else DR_GM_FWD2(KK, 1);           \
  } while (0)
  DR_GM_DISPATCH(DR_GM_FWD)
#undef DR_GM_FWD
#undef DR_GM_FWD2
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_gate_mix_backward(const float* h, int64_t ld_h, const float* gates,
                                    const float* go, int64_t ld_go, const uint32_t* select_bits,
                                    int64_t B, int64_t K, int64_t E, int64_t H, float* grad_z,
                                    float* grad_h, void* stream) {
  const char* what = "dr_gate_mix_backward";
  GmSelect sel;
  if (int rc = gm_check(what, B, K, E, H, select_bits, sel)) return rc;
  if (int rc = gm_stride(what, "ld_h", ld_h, E * H)) return rc;
  if (int rc = gm_stride(what, "ld_go", ld_go, K * H)) return rc;
  DR_REQUIRE(h && gates && go && grad_z && grad_h, DR_INVALID_ARGUMENT,
             "%s (gate_mix): a required pointer is null", what);
  DR_REQUIRE(aligned16(h) && aligned16(gates) && aligned16(go) && aligned16(grad_z) &&
                 aligned16(grad_h),
             DR_INVALID_ARGUMENT,
             "%s (gate_mix): h, gates, go and the gradients must be 16-byte aligned", what);
  if (B == 0) return DR_OK;
  const GmGeometry g = gm_geometry(K, E, H);
  const dim3 grid((unsigned)ceil_div(B, g.tile)), block(g.waves * 64);
#define DR_GM_BWD2(KK, CPL)                                                                   \
  hipLaunchKernelGGL((gate_mix_backward_kernel<KK, CPL>), grid, block, 2 * g.lds, S(stream), h, \
                     ld_h, gates, go, ld_go, sel, B, (int)E, (int)H, g.ll, grad_z, grad_h)
#define DR_GM_BWD(KK)                 \
  do {                                \
    if (H > 256) DR_GM_BWD2(KK, 2);   \
    else DR_GM_BWD2(KK, 1);           \
  } while (0)
  DR_GM_DISPATCH(DR_GM_BWD)
#undef DR_GM_BWD
#undef DR_GM_BWD2
  DR_LAUNCH_CHECK();
  return DR_OK;
}
