// cin.hip -- one layer of xDeepFM's Compressed Interaction Network, forward
// and backward, fp32 on the matrix cores.
//
//   out[b, h, d] = bias[h] + sum_{i < Hk, j < m} W[h, i, j] xk[b, i, d] x0[b, j, d]
//
// With the flattened column n = b D + d this is the GEMM out[h, n] = sum_k
// W[h, k] Z[k, n] over k = (i, j) whose operand Z[(i, j), n] = xk[n, i] x0[n, j]
// is formed in registers on the way into the MFMA and never stored; so is
// its counterpart T of the backward.  Every product is
// v_mfma_f32_16x16x4_f32: lane (r, g) = (lane % 16, lane / 16) supplies
// A[row r][k g] and B[k g][column r], and accumulator register c of the lane
// is element [4 g + c][r].  A tile of 16 columns is 16 consecutive n, whatever
// D: whole samples, a part of one, or the end of one and the start of the
// next.  A column at or past B D reads column B D - 1 and is not stored.
//
// Forward (one launch): a block of 8 waves takes 128 columns, a wave 16 of them
// and all ceil(Hn / 16) row tiles.  K runs over steps s = i MT + t (MT = ceil(m
// / 4)); step s is the four j = 4 t + g of one i.  The lane's x0[n_r][4 t + g]
// for every t sit in a lane-private strip of LDS, xk[n_r][i] is loaded as i
// advances (one ahead), the B operand of a step is their product, shared by
// the step's row tiles.  W comes through LDS in stages of KS steps, laid out
// [step][h][g] so that the 64 A reads of a wave are 64 consecutive floats; the
// next stage is fetched into registers while this one is multiplied (two
// buffers, one barrier a stage).  Padded j, rows past Hn and steps past the
// last are staged as zeros.  An accumulator chain is cut every 64 steps (256
// terms) and the chains are added in order: one chain over the up to 16 384
// terms of a row misses the fp64 bound at the largest shapes.
//
// Input gradients (one launch): T[(i, j), n] = sum_h W[h, i, j] grad_out[n, h].
// A 16-row tile is 4 i by 4 j (row 4 g + c = (i0 + g, 4 t + c)), so register c
// of lane (r, g) is T[(i0 + g, 4 t + c), n_r]: grad_xk[n_r][i0 + g] is a sum
// inside the lane (fmaf over ascending j), grad_x0[n_r][4 t + c] accumulates
// in the lane over its i and is summed over g once at the end (xor 16, then
// xor 32).  A wave holds the MT tiles of one i0 at a time; W transposed comes
// through LDS in panels of (4 i, HS steps of 4 h, all j), laid out [step][t]
// [r][g].
//
// Weight gradient (one launch and a finishing launch): grad_W[h, (i, j)] =
// sum_n grad_out[n, h] Z[n, (i, j)].  A block owns a band of 256 flattened
// (i, j) and all h, and one of S slices of the columns; a wave two 16-wide
// tiles of the band.  grad_out, the band's rows of xk and x0 are staged
// transposed, [step][row][g], four columns a step, and both operands read
// from there.  The block of band 0 also sums grad_out's staged rows: that is
// grad_bias's partial.  S depends on (B D, Hn, Hk, m) alone; the finishing
// kernel adds the S partials in ascending order.  No atomics anywhere.
#include "dr_common.h"

namespace dr {
namespace {

constexpr int CIN_MAX_D = 64, CIN_MAX_M = 64, CIN_MAX_H = 256;
constexpr int CIN_THREADS = 512, CIN_WAVES = CIN_THREADS / 64;
constexpr int CIN_STAGE = 4096;            // floats of one W stage buffer (16 KB)
constexpr int CIN_PRE = 8;                 // staged floats a thread carries
constexpr int CIN_BAND = 256;              // (i, j) columns of a weight-gradient block
constexpr int CIN_WG_STAGE = 4608;         // floats of one weight-gradient stage buffer
constexpr int CIN_WG_PRE = 9;
constexpr int CIN_CUS = 256;               // the weight gradient's grid aims at one block a CU
constexpr int CIN_MAX_SLICES = 32;
constexpr size_t CIN_MAX_PARTIAL_BYTES = size_t(64) << 20;

typedef float mf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ mf4 mma(float a, float b, mf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Column n of the flattened batch: its sample and its place in it; a column
// past the end reads the last one.
struct Col {
  int64_t b;
  int d;
  bool on;
};
__device__ __forceinline__ Col column(int64_t n, int64_t BD, int D) {
  Col c;
  c.on = n < BD;
  const uint32_t nn = (uint32_t)(c.on ? n : BD - 1);
  const uint32_t b = nn / (uint32_t)D;
  c.b = b;
  c.d = (int)(nn - b * (uint32_t)D);
  return c;
}

struct CinPlan {
  int lks;        // forward: log2 of the steps of a W stage
  int lhs, lmt;   // input gradients: log2 of the h steps of a panel, of MT rounded up
  int lnk;        // weight gradient: log2 of the column steps of a stage
  int bands, slices;
  int64_t part;   // floats of one slice's partial: grad_W, then grad_bias
};

CinPlan cin_plan(int64_t BD, int64_t m, int64_t Hk, int64_t Hn) {
  CinPlan p;
  const int HnP = (int)ceil_div(Hn, 16) * 16, MT = (int)ceil_div(m, 4);
  p.lks = 0;
  while ((2 << p.lks) * HnP <= 1024 && p.lks < 6) ++p.lks;
  p.lmt = 0;
  while ((1 << p.lmt) < MT) ++p.lmt;
  p.lhs = 0;
  while (p.lhs < 3 && ((2 << p.lhs) << p.lmt) <= 64) ++p.lhs;
  const int64_t Q = Hk * m;
  const int64_t ni = CIN_BAND / m + 2 < Hk ? CIN_BAND / m + 2 : Hk;
  p.lnk = HnP + ni + m <= 256 ? 2 : 1;
  p.bands = (int)ceil_div(Q, CIN_BAND);
  p.part = Hn * Q + Hn;
  const int64_t stages = ceil_div(ceil_div(BD, 4), (int64_t)1 << p.lnk);
  int64_t S = CIN_CUS / p.bands;
  if (S > CIN_MAX_SLICES) S = CIN_MAX_SLICES;
  if (S > stages) S = stages;
  while (S > 1 && (size_t)S * p.part * sizeof(float) > CIN_MAX_PARTIAL_BYTES) --S;
  p.slices = S < 1 ? 1 : (int)S;
  return p;
}

template <int RTM>
__global__ __launch_bounds__(CIN_THREADS) void cin_forward_kernel(
    const float* __restrict__ x0, const float* __restrict__ xk, const float* __restrict__ W,
    const float* __restrict__ bias, int64_t BD, int D, int m, int Hk, int Hn, int lks,
    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int MT = (m + 3) >> 2, RT = (Hn + 15) >> 4, HnP = RT * 16, KS = 1 << lks;
  const int NS = Hk * MT, NST = (NS + KS - 1) >> lks;
  float* x0s = lds + 2 * CIN_STAGE + wave * MT * 64;        // [t][lane]: the lane's own strip

  const int64_t tile = (int64_t)blockIdx.x * CIN_WAVES + wave;
  const bool live = tile * 16 < BD;                          // (uniform over the wave)
  const Col at = column(tile * 16 + r, BD, D);
  const float* x0c = x0 + at.b * m * D + at.d;
  const float* xkc = xk + at.b * Hk * D + at.d;
  for (int t = 0; t < MT; ++t) {
    const int j = 4 * t + g;
    x0s[t * 64 + lane] = j < m ? gld(x0c + (int64_t)j * D) : 0.0f;
  }

  // the thread's part of a stage: step sl, k-slot gg, rows hrow0 + q hstep
  const int sub = tid & ((4 << lks) - 1), sl = sub >> 2, gg = sub & 3;
  const int hrow0 = tid >> (lks + 2), hstep = CIN_THREADS >> (lks + 2);
  float pre[CIN_PRE];
  auto fetch = [&](int st) {
    const int s = (st << lks) + sl, i = s / MT, j = 4 * (s - i * MT) + gg;
    const bool ok = s < NS && j < m;
    const float* wp = W + (int64_t)(ok ? i : 0) * m + (ok ? j : 0);
#pragma unroll
    for (int q = 0; q < CIN_PRE; ++q) {
      const int h = hrow0 + q * hstep;
      pre[q] = ok && h < Hn ? gld(wp + (int64_t)h * Hk * m) : 0.0f;
    }
  };
  auto put = [&](float* buf) {
#pragma unroll
    for (int q = 0; q < CIN_PRE; ++q) {
      const int h = hrow0 + q * hstep;
      if (h < HnP) buf[(sl * HnP + h) * 4 + gg] = pre[q];
    }
  };

  // acc: the running chain of at most 64 steps (256 terms); tot: the sum of the chains
  mf4 acc[RTM], tot[RTM];
#pragma unroll
  for (int a = 0; a < RTM; ++a) acc[a] = tot[a] = mf4{0.f, 0.f, 0.f, 0.f};
  const int flush = (1 << (6 - lks)) - 1;                    // stages of a chain, less one
  fetch(0);
  put(lds);
  __syncthreads();
  int i = 0, t = 0;
  float xc = gld(xkc), xn = gld(xkc + (int64_t)(Hk > 1 ? 1 : 0) * D);
  for (int st = 0; st < NST; ++st) {
    if (st + 1 < NST) fetch(st + 1);
    if (live) {
      const float* wr = lds + (st & 1) * CIN_STAGE + r * 4 + g;   // [u][h = r][g]
      const int left = NS - (st << lks), steps = left < KS ? left : KS;
      for (int u = 0; u < steps; ++u) {
        const float b = xc * x0s[t * 64 + lane];
        const float* wa = wr + u * HnP * 4;
#pragma unroll
        for (int a = 0; a < RTM; ++a)
          if (a < RT) acc[a] = mma(wa[a * 64], b, acc[a]);
        if (++t == MT) {
          t = 0;
          ++i;
          xc = xn;
          xn = gld(xkc + (int64_t)(i + 1 < Hk ? i + 1 : Hk - 1) * D);
        }
      }
      if ((st & flush) == flush || st + 1 == NST) {
#pragma unroll
        for (int a = 0; a < RTM; ++a) {
          tot[a] += acc[a];
          acc[a] = mf4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    if (st + 1 < NST) put(lds + ((st + 1) & 1) * CIN_STAGE);
    __syncthreads();
  }

  if (!live || !at.on) return;
  float* oc = out + at.b * Hn * D + at.d;
#pragma unroll
  for (int a = 0; a < RTM; ++a) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int h = 16 * a + 4 * g + c;
      if (a < RT && h < Hn) {
        const float v = tot[a][c];
        gst(oc + (int64_t)h * D, bias != nullptr ? v + gld(bias + h) : v);
      }
    }
  }
}

template <int MTM>
__global__ __launch_bounds__(CIN_THREADS) void cin_input_grad_kernel(
    const float* __restrict__ x0, const float* __restrict__ xk, const float* __restrict__ W,
    const float* __restrict__ go, int64_t BD, int D, int m, int Hk, int Hn, int lhs, int lmt,
    float* __restrict__ gxk, float* __restrict__ gx0) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int MT = (m + 3) >> 2, HQ = (Hn + 3) >> 2, HS = 1 << lhs;
  const int NHP = (HQ + HS - 1) >> lhs, NP = ((Hk + 3) >> 2) * NHP;
  float* x0s = lds + 2 * CIN_STAGE + wave * MT * 64;        // [t][r][c] = x0[n_r][4 t + c]

  const int64_t tile = (int64_t)blockIdx.x * CIN_WAVES + wave;
  const bool live = tile * 16 < BD;
  const Col at = column(tile * 16 + r, BD, D);
  const float* x0c = x0 + at.b * m * D + at.d;
  const float* xkc = xk + at.b * Hk * D + at.d;
  const float* goc = go + at.b * Hn * D + at.d;
  for (int t = 0; t < MT; ++t) {
    const int j = 4 * t + g;
    x0s[(t * 16 + r) * 4 + g] = j < m ? gld(x0c + (int64_t)j * D) : 0.0f;
  }

  // element e = tid + 512 q of a panel: [hs][gg][ri][t (padded to 1 << lmt)][rj]
  const int total = (HS << lmt) * 64;
  float pre[CIN_PRE];
  auto fetch = [&](int p) {
    const int ig = p / NHP, i0 = 4 * ig, hs0 = (p - ig * NHP) << lhs;
#pragma unroll
    for (int q = 0; q < CIN_PRE; ++q) {
      const int e = tid + CIN_THREADS * q;
      const int rj = e & 3, t = (e >> 2) & ((1 << lmt) - 1), rest = e >> (2 + lmt);
      const int ri = rest & 3, gq = (rest >> 2) & 3, hs = rest >> 4;
      const int h = 4 * (hs0 + hs) + gq, i = i0 + ri, j = 4 * t + rj;
      const bool ok = e < total && h < Hn && i < Hk && j < m;
      pre[q] = ok ? gld(W + ((int64_t)h * Hk + i) * m + j) : 0.0f;
    }
  };
  auto put = [&](float* buf) {
#pragma unroll
    for (int q = 0; q < CIN_PRE; ++q) {
      const int e = tid + CIN_THREADS * q;
      const int rj = e & 3, t = (e >> 2) & ((1 << lmt) - 1), rest = e >> (2 + lmt);
      const int ri = rest & 3, gq = (rest >> 2) & 3, hs = rest >> 4;
      if (e < total && t < MT) buf[((hs * MT + t) * 16 + ri * 4 + rj) * 4 + gq] = pre[q];
    }
  };

  mf4 acc[MTM], sx0[MTM];
#pragma unroll
  for (int t = 0; t < MTM; ++t) acc[t] = sx0[t] = mf4{0.f, 0.f, 0.f, 0.f};
  float xki = 0.0f;
  fetch(0);
  put(lds);
  __syncthreads();
  for (int p = 0; p < NP; ++p) {
    if (p + 1 < NP) fetch(p + 1);
    if (live) {
      const int ig = p / NHP, i0 = 4 * ig, hp = p - ig * NHP, hs0 = hp << lhs;
      const float* wr = lds + (p & 1) * CIN_STAGE + r * 4 + g;
      if (hp == 0) {
        xki = i0 + g < Hk ? gld(xkc + (int64_t)(i0 + g) * D) : 0.0f;
#pragma unroll
        for (int t = 0; t < MTM; ++t) acc[t] = mf4{0.f, 0.f, 0.f, 0.f};
      }
      // the B operand grad_out[n_r][4 (hs0 + u) + g], one step ahead (0 past Hn)
      const int steps = HQ - hs0 < HS ? HQ - hs0 : HS;
      auto go_at = [&](int u) {
        const int h = 4 * (hs0 + u) + g;
        return h < Hn ? gld(goc + (int64_t)h * D) : 0.0f;
      };
      float gnext = go_at(0);
#pragma unroll 1
      for (int u = 0; u < steps; ++u) {
        const float gcur = gnext;
        gnext = go_at(u + 1);
        const float* wa = wr + u * MT * 64;
#pragma unroll
        for (int t = 0; t < MTM; ++t)
          if (t < MT) acc[t] = mma(wa[t * 64], gcur, acc[t]);
      }
      if (hp == NHP - 1) {               // T of (i0 + g, every j) is complete
        float gk = 0.0f;
#pragma unroll
        for (int t = 0; t < MTM; ++t) {
          if (t < MT) {
            const float4 xv = *reinterpret_cast<const float4*>(x0s + (t * 16 + r) * 4);
            gk = fmaf(acc[t][0], xv.x, gk);
            gk = fmaf(acc[t][1], xv.y, gk);
            gk = fmaf(acc[t][2], xv.z, gk);
            gk = fmaf(acc[t][3], xv.w, gk);
#pragma unroll
            for (int c = 0; c < 4; ++c) sx0[t][c] = fmaf(acc[t][c], xki, sx0[t][c]);
          }
        }
        if (at.on && i0 + g < Hk) gst(gxk + (at.b * Hk + i0 + g) * D + at.d, gk);
      }
    }
    if (p + 1 < NP) put(lds + ((p + 1) & 1) * CIN_STAGE);
    __syncthreads();
  }

  if (!live) return;
#pragma unroll
  for (int t = 0; t < MTM; ++t) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = sx0[t][c];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int j = 4 * t + c;
      if (g == 0 && at.on && j < m) gst(gx0 + (at.b * m + j) * D + at.d, v);
    }
  }
}

template <int RTM>
__global__ __launch_bounds__(CIN_THREADS) void cin_weight_grad_kernel(
    const float* __restrict__ x0, const float* __restrict__ xk, const float* __restrict__ go,
    int64_t BD, int D, int m, int Hk, int Hn, int lnk, int64_t part, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float lds[2 * CIN_WG_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int RT = (Hn + 15) >> 4, HnP = RT * 16, NK = 1 << lnk, Q = Hk * m;
  const int q0 = blockIdx.x * CIN_BAND, qe = q0 + CIN_BAND < Q ? q0 + CIN_BAND : Q;
  const int i_lo = q0 / m, NI = (qe - 1) / m - i_lo + 1, rows = HnP + NI + m;
  const int64_t stages = ceil_div(ceil_div(BD, 4), NK), per = ceil_div(stages, gridDim.y);
  const int64_t first = blockIdx.y * per;
  const int64_t last = first + per < stages ? first + per : stages;

  // the thread's part of a stage: column step ks, k-slot gg, rows row0 + q rstep
  const int sub = tid & ((4 << lnk) - 1), ks = sub >> 2, gg = sub & 3;
  const int row0 = tid >> (lnk + 2), rstep = CIN_THREADS >> (lnk + 2);
  float pre[CIN_WG_PRE];
  auto fetch = [&](int64_t st) {
    const Col c = column(((st << lnk) + ks) * 4 + gg, BD, D);
#pragma unroll
    for (int q = 0; q < CIN_WG_PRE; ++q) {
      const int row = row0 + q * rstep;
      const float* p = nullptr;
      if (row < Hn) p = go + (c.b * Hn + row) * D;
      else if (row >= HnP && row < HnP + NI) p = xk + (c.b * Hk + i_lo + row - HnP) * D;
      else if (row >= HnP + NI && row < rows) p = x0 + (c.b * m + row - HnP - NI) * D;
      pre[q] = c.on && p != nullptr ? gld(p + c.d) : 0.0f;
    }
  };
  auto put = [&](float* buf) {
#pragma unroll
    for (int q = 0; q < CIN_WG_PRE; ++q) {
      const int row = row0 + q * rstep;
      if (row < rows) buf[(ks * rows + row) * 4 + gg] = pre[q];
    }
  };

  // the wave's two tiles of the band: lane r holds column q = (i, j) of each
  int xi[2], xj[2];
  bool mine = false;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int qt = q0 + (wave * 2 + u) * 16;
    const int q = qt + r < Q ? qt + r : q0;
    mine = mine || qt < Q;
    xi[u] = (HnP + q / m - i_lo) * 4 + g;
    xj[u] = (HnP + NI + q % m) * 4 + g;
  }
  mf4 acc[2][RTM];
#pragma unroll
  for (int a = 0; a < RTM; ++a) acc[0][a] = acc[1][a] = mf4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.0f;

  if (first < last) {
    fetch(first);
    put(lds);
  }
  __syncthreads();
  for (int64_t st = first; st < last; ++st) {
    const float* buf = lds + ((st - first) & 1) * CIN_WG_STAGE;
    if (st + 1 < last) fetch(st + 1);
    if (mine) {
      for (int k = 0; k < NK; ++k) {
        const float* base = buf + k * rows * 4;
        const float b0 = base[xi[0]] * base[xj[0]], b1 = base[xi[1]] * base[xj[1]];
        const float* ga = base + r * 4 + g;
#pragma unroll
        for (int a = 0; a < RTM; ++a) {
          if (a < RT) {
            const float av = ga[a * 64];
            acc[0][a] = mma(av, b0, acc[0][a]);
            acc[1][a] = mma(av, b1, acc[1][a]);
          }
        }
      }
    }
    if (blockIdx.x == 0 && tid < Hn) {
      for (int k = 0; k < NK; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(buf + (k * rows + tid) * 4);
        bsum = (((bsum + v.x) + v.y) + v.z) + v.w;
      }
    }
    if (st + 1 < last) put(lds + ((st + 1 - first) & 1) * CIN_WG_STAGE);
    __syncthreads();
  }

  float* pw = ws + (int64_t)blockIdx.y * part;
  if (blockIdx.x == 0 && tid < Hn) gst(pw + (int64_t)Hn * Q + tid, bsum);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = q0 + (wave * 2 + u) * 16 + r;
#pragma unroll
    for (int a = 0; a < RTM; ++a) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int h = 16 * a + 4 * g + c;
        if (a < RT && h < Hn && q < Q) gst(pw + (int64_t)h * Q + q, acc[u][a][c]);
      }
    }
  }
}

// grad_W | grad_bias from the slices' partials, ascending.
__global__ __launch_bounds__(256) void cin_finish_kernel(const float* __restrict__ ws, int slices,
                                                         int64_t part, int64_t nw,
                                                         float* __restrict__ gw,
                                                         float* __restrict__ gbias) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= part) return;
  float v = gld(ws + e);
  for (int s = 1; s < slices; ++s) v += gld(ws + (int64_t)s * part + e);
  if (e < nw) gst(gw + e, v);
  else if (gbias != nullptr) gst(gbias + (e - nw), v);
}

int cin_check(const char* what, int64_t B, int64_t m, int64_t Hk, int64_t Hn, int64_t D) {
  DR_REQUIRE(D >= 1 && D <= CIN_MAX_D, DR_INVALID_ARGUMENT,
             "%s (cin): embedding width %lld is outside [1, %d]", what, (long long)D, CIN_MAX_D);
  DR_REQUIRE(m >= 1 && m <= CIN_MAX_M, DR_INVALID_ARGUMENT,
             "%s (cin): fields %lld is outside [1, %d]", what, (long long)m, CIN_MAX_M);
  DR_REQUIRE(Hk >= 1 && Hk <= CIN_MAX_H && Hn >= 1 && Hn <= CIN_MAX_H, DR_INVALID_ARGUMENT,
             "%s (cin): maps in %lld / out %lld are outside [1, %d]", what, (long long)Hk,
             (long long)Hn, CIN_MAX_H);
  DR_REQUIRE(B >= 0 && B * D <= (int64_t(1) << 31) - 1, DR_INVALID_ARGUMENT,
             "%s (cin): batch %lld x width %lld is outside [0, 2^31)", what, (long long)B,
             (long long)D);
  return DR_OK;
}

}  // namespace
}  // namespace dr

using namespace dr;

#define DR_CIN_ROWS(RT, LAUNCH)  \
  if ((RT) <= 4) LAUNCH(4);      \
  else if ((RT) <= 8) LAUNCH(8); \
  else LAUNCH(16)

extern "C" size_t dr_cin_workspace_size(int64_t B, int64_t m, int64_t Hk, int64_t Hn, int64_t D) {
  if (B <= 0 || m < 1 || m > CIN_MAX_M || Hk < 1 || Hk > CIN_MAX_H || Hn < 1 ||
      Hn > CIN_MAX_H || D < 1 || D > CIN_MAX_D)
    return 0;
  const CinPlan p = cin_plan(B * D, m, Hk, Hn);
  return (size_t)p.slices * (size_t)p.part * sizeof(float);
}

extern "C" int dr_cin_forward(const float* x0, const float* xk, const float* weight,
                              const float* bias, int64_t B, int64_t m, int64_t Hk, int64_t Hn,
                              int64_t D, float* out, void* stream) {
  const char* what = "dr_cin_forward";
  if (int rc = cin_check(what, B, m, Hk, Hn, D)) return rc;
  DR_REQUIRE(x0 && xk && weight && out, DR_INVALID_ARGUMENT,
             "%s (cin): a required pointer is null", what);
  if (B == 0) return DR_OK;
  const int64_t BD = B * D;
  const CinPlan p = cin_plan(BD, m, Hk, Hn);
  const int MT = (int)ceil_div(m, 4), RT = (int)ceil_div(Hn, 16);
  const dim3 grid((unsigned)ceil_div(ceil_div(BD, 16), CIN_WAVES)), block(CIN_THREADS);
  const size_t lds = (size_t)(2 * CIN_STAGE + CIN_WAVES * MT * 64) * sizeof(float);
#define DR_CIN_FWD(RR)                                                                         \
  hipLaunchKernelGGL(cin_forward_kernel<RR>, grid, block, lds, S(stream), x0, xk, weight, bias, \
                     BD, (int)D, (int)m, (int)Hk, (int)Hn, p.lks, out)
  DR_CIN_ROWS(RT, DR_CIN_FWD);
#undef DR_CIN_FWD
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_cin_backward(const float* x0, const float* xk, const float* weight,
                               const float* grad_out, int64_t B, int64_t m, int64_t Hk,
                               int64_t Hn, int64_t D, float* grad_xk, float* grad_x0,
                               float* grad_weight, float* grad_bias, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const char* what = "dr_cin_backward";
  if (int rc = cin_check(what, B, m, Hk, Hn, D)) return rc;
  DR_REQUIRE(x0 && xk && weight && grad_out && grad_xk && grad_x0 && grad_weight,
             DR_INVALID_ARGUMENT, "%s (cin): a required pointer is null", what);
  DR_REQUIRE(grad_xk != grad_x0, DR_INVALID_ARGUMENT,
             "%s (cin): grad_xk and grad_x0 must be two buffers", what);
  if (B == 0) return DR_OK;
  const size_t need = dr_cin_workspace_size(B, m, Hk, Hn, D);
  DR_REQUIRE(workspace != nullptr && workspace_bytes >= need, DR_INVALID_ARGUMENT,
             "%s (cin): workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  const int64_t BD = B * D;
  const CinPlan p = cin_plan(BD, m, Hk, Hn);
  const int MT = (int)ceil_div(m, 4), RT = (int)ceil_div(Hn, 16);
  const dim3 block(CIN_THREADS);
  {
    const dim3 grid((unsigned)ceil_div(ceil_div(BD, 16), CIN_WAVES));
    const size_t lds = (size_t)(2 * CIN_STAGE + CIN_WAVES * MT * 64) * sizeof(float);
#define DR_CIN_DX(MM)                                                                          \
  hipLaunchKernelGGL(cin_input_grad_kernel<MM>, grid, block, lds, S(stream), x0, xk, weight,   \
                     grad_out, BD, (int)D, (int)m, (int)Hk, (int)Hn, p.lhs, p.lmt, grad_xk,    \
                     grad_x0)
    if (MT <= 2) DR_CIN_DX(2);
    else if (MT <= 8) DR_CIN_DX(8);
    else DR_CIN_DX(16);
#undef DR_CIN_DX
    DR_LAUNCH_CHECK();
  }
  float* ws = static_cast<float*>(workspace);
  {
    const dim3 grid((unsigned)p.bands, (unsigned)p.slices);
#define DR_CIN_DW(RR)                                                                          \
  hipLaunchKernelGGL(cin_weight_grad_kernel<RR>, grid, block, 0, S(stream), x0, xk, grad_out,  \
                     BD, (int)D, (int)m, (int)Hk, (int)Hn, p.lnk, p.part, ws)
    DR_CIN_ROWS(RT, DR_CIN_DW);
#undef DR_CIN_DW
    DR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cin_finish_kernel, dim3((unsigned)ceil_div(p.part, 256)), dim3(256), 0,
                     S(stream), ws, p.slices, p.part, Hn * Hk * m, grad_weight, grad_bias);
  DR_LAUNCH_CHECK();
  return DR_OK;
}
