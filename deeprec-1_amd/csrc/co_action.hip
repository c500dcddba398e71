// co_action.hip -- CAN's co-action unit: a per-sample micro-MLP over the
// positions of a history, forward and backward, fp32 on the matrix cores
// (DESIGN section 30).
//
//   widths (d0, ..., dL), 1 <= L <= 3, every d a multiple of 4 in [4, 32]
//   param [B, P]  row b: per set, for j = 1..L: W_j [d(j-1), d(j)] row-major, then b_j [d(j)]
//   for p = 1..orders:  a_0 = his ** p;  (W, b) = set p - 1 (order_indep) or set 0
//     for j = 1..L:     a_j = a_(j-1) W_j + b_j;  j < L: a_j = tanh(a_j)
//   out[b, (p, j, f)] = sum_t mask[b, t] a_j[b, t, f]
//
// One wave owns one sample for the whole launch; the waves of a block share
// nothing and never synchronise.  No LDS, no workspace, no atomics: every sum
// runs in an order fixed by the shapes, so a sample's bits do not depend on its
// batch and runs repeat.
//
// Every product is v_mfma_f32_16x16x4_f32: lane (r, g) = (lane % 16, lane / 16)
// supplies A[row r][k g] and B[k g][column r], and accumulator register i of
// the lane is element [4 g + i][r].  Positions are cut into tiles of 16 and a
// quantity of a tile lives in registers in one of two layouts (n, a: 16-wide
// blocks of features, at most two of them):
//
//   T layout  v[n][c] of lane (r, g) = v[position t0 + r][feature 16 n + 4 g + c]
//   U layout  v[n][i] of lane (r, g) = v[position t0 + 4 g + i][feature 16 n + r]
//
// his is loaded in the T layout, one float4 per lane and block.  For the
// contraction step (n, c) the lane's k slot g stands for feature 16 n + 4 g +
// c, so the B operand of a layer is its input as it stands, and with the
// weight fragment
//
//   f[j][a][n][c]  of lane (r, g) = W_j[16 n + 4 g + c][16 a + r]
//
// as A the accumulator is a_j transposed, feature 16 a + 4 g + i of position r
// in register i: the T layout again.  After tanh in registers it is the next
// layer's B operand.  Slots past a width are zero in the fragments, so widths
// such as 8, 12 and 20 take no path of their own; a block that is empty as a
// whole is skipped.  The fragments are loaded once per (sample, set): 16 L
// registers at most, with the bias fragment 4 L more per block.
//
// Forward: the powers his ** p come from the loaded fragment (repeated
// products), the L layers run in registers, every layer's activations times
// the lane's position's mask accumulate over the tiles in registers, and at the
// end one xor butterfly (8, 4, 2, 1) over the 16 lanes of a DPP row sums the
// positions; lane r = 0 of the row stores four features.  A position with mask
// 0, or past T, reads nothing (its his is taken as 0), and a tile without a
// live position is not visited.
//
// Backward (recomputes, nothing was saved).  Per tile and order:
//   delta_j    = mask go[(p, j)] + delta'_(j+1) W_(j+1)^T      (j < L)
//   delta'_j   = delta_j (1 - a_j^2)  (j < L),  delta'_L = mask go[(p, L)]
//   grad_W_j  += a_(j-1)^T delta'_j,  grad_b_j += sum_t delta'_j
//   grad_his  += p his^(p-1) delta_0
// The chain back uses the same lane map with the second fragment
//   wb[j][n][a][i] of lane (r, g) = W_j[16 n + r][16 a + 4 g + i]
// as A and delta'_j (T layout) as B: the accumulator is delta_(j-1) in the T
// layout.  grad_W_j contracts over positions, which needs both operands in
// the U layout.  They come from the same products with the MFMA operands
// swapped (as mha.hip's backward does): mma(a_(j-1) T, f) is a_j in the U
// layout and mma(delta'_j T, wb) is delta_(j-1) in the U layout, at the price
// of a second tanh; his in the U layout is a second (scalar) load of the tile,
// which L1 serves.  Then grad_W_j[a][n] += mma(a_(j-1) U, delta'_j U) over the
// four steps i, and the accumulator has the layout of f.  grad_W_j and
// grad_b_j accumulate in registers over the tiles and, for shared weights,
// over the orders, and are stored once; grad_b_j takes the butterfly of the
// forward.  grad_his is stored as float4 per tile, exact zeros where the mask
// is 0.  With order_indep the sets are the outer loop (one set's fragments
// live at a time) and the sets after the first add to the grad_his the same
// lane stored before.
#include "dr_common.h"

namespace dr {
namespace {

constexpr int CO_MAX_L = 3, CO_MAX_D = 32, CO_MAX_ORDERS = 4;
constexpr int CO_THREADS = 256, CO_WAVES = CO_THREADS / 64;

typedef float mf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ mf4 mma(float a, float b, mf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ mf4 ld4(const float* p) {
  return *gp(reinterpret_cast<const mf4*>(p));
}
__device__ __forceinline__ void st4(float* p, mf4 v) { *gp(reinterpret_cast<mf4*>(p)) = v; }
__device__ __forceinline__ mf4 splat(float v) { return mf4{v, v, v, v}; }
__device__ __forceinline__ mf4 tanh4(mf4 v) {
  return mf4{tanhf(v[0]), tanhf(v[1]), tanhf(v[2]), tanhf(v[3])};
}
// The sum over the 16 lanes of a DPP row, in every lane of it.
__device__ __forceinline__ mf4 row_sum(mf4 v) {
#pragma unroll
  for (int s = 8; s >= 1; s >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += __shfl_xor(v[i], s, 64);
  }
  return v;
}

struct CoPlan {
  int L, orders, bias, indep;
  int d[CO_MAX_L + 1];
  int woff[CO_MAX_L], boff[CO_MAX_L];   // W_j, b_j of layer j + 1 inside a set
  int ooff[CO_MAX_L];                   // layer j + 1's slice inside an order's part of out
  int set_len, S, P;                    // floats of a set; sum_{j >= 1} d_j; floats of a row
};

// Whether block n of a width-d quantity holds any feature (always, with one block).
template <int NT>
__device__ __forceinline__ bool has(int n, int d) {
  return NT == 1 || 16 * n < d;
}

// xm1 = x ** (p - 1) and xp = x ** p by repeated products.
template <int NT>
__device__ __forceinline__ void powers(const mf4 (&x)[NT], int p, mf4 (&xm1)[NT], mf4 (&xp)[NT]) {
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    mf4 v = splat(1.0f);
    for (int k = 1; k < p; ++k) v *= x[n];
    xm1[n] = v;
    xp[n] = v * x[n];
  }
}

// f and the T-layout bias of one set (zeros past the widths).
template <int L, int NT>
__device__ __forceinline__ void load_forward_fragments(const float* set, const CoPlan& pl, int r,
                                                       int g, mf4 (&f)[L][NT][NT],
                                                       mf4 (&bt)[L][NT]) {
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const int din = pl.d[j], dout = pl.d[j + 1];
    const float* w = set + pl.woff[j];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      const int col = 16 * a + r;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int row = 16 * n + 4 * g + c;
          f[j][a][n][c] = row < din && col < dout ? gld(w + row * dout + col) : 0.0f;
        }
      }
      const int f0 = 16 * a + 4 * g;
      bt[j][a] = pl.bias && f0 < dout ? ld4(set + pl.boff[j] + f0) : splat(0.0f);
    }
  }
}

template <int L, int NT>
__global__ __launch_bounds__(CO_THREADS) void co_action_forward_kernel(
    const float* __restrict__ param, int64_t ld_p, const float* __restrict__ his, int64_t ld_h,
    const float* __restrict__ mask, int64_t B, int T, CoPlan pl, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * CO_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;                                        // (uniform over the wave)
  const float* hb = his + b * T * ld_h;
  const float* mb = mask + b * T;
  float* ob = out + b * pl.orders * pl.S;
  const int n_sets = pl.indep ? pl.orders : 1, ord_in = pl.indep ? 1 : pl.orders;
  const int ntiles = (T + 15) >> 4;

  for (int set = 0; set < n_sets; ++set) {
    mf4 f[L][NT][NT], bt[L][NT];
    load_forward_fragments<L, NT>(param + b * ld_p + (int64_t)set * pl.set_len, pl, r, g, f, bt);
    mf4 pool[CO_MAX_ORDERS][L][NT];
#pragma unroll
    for (int q = 0; q < CO_MAX_ORDERS; ++q)
#pragma unroll
      for (int j = 0; j < L; ++j)
#pragma unroll
        for (int a = 0; a < NT; ++a) pool[q][j][a] = splat(0.0f);

    for (int tile = 0; tile < ntiles; ++tile) {
      const int t = tile * 16 + r;
      const float m = t < T ? gld(mb + t) : 0.0f;
      const bool on = m != 0.0f;
      if (!__any(on)) continue;
      mf4 x[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int f0 = 16 * n + 4 * g;
        x[n] = on && f0 < pl.d[0] ? ld4(hb + (int64_t)t * ld_h + f0) : splat(0.0f);
      }
#pragma unroll
      for (int q = 0; q < CO_MAX_ORDERS; ++q) {
        if (q < ord_in) {
          mf4 xm1[NT], h[NT];
          powers<NT>(x, pl.indep ? set + 1 : q + 1, xm1, h);
#pragma unroll
          for (int j = 0; j < L; ++j) {
            mf4 y[NT];
#pragma unroll
            for (int a = 0; a < NT; ++a) {
              y[a] = bt[j][a];
              if (has<NT>(a, pl.d[j + 1])) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                  if (has<NT>(n, pl.d[j])) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) y[a] = mma(f[j][a][n][c], h[n][c], y[a]);
                  }
                }
                if (j + 1 < L) y[a] = tanh4(y[a]);
                pool[q][j][a] += y[a] * m;
              }
            }
#pragma unroll
            for (int a = 0; a < NT; ++a) h[a] = y[a];
          }
        }
      }
    }

#pragma unroll
    for (int q = 0; q < CO_MAX_ORDERS; ++q) {
      if (q < ord_in) {
        float* oq = ob + (int64_t)(pl.indep ? set : q) * pl.S;
#pragma unroll
        for (int j = 0; j < L; ++j) {
#pragma unroll
          for (int a = 0; a < NT; ++a) {
            const mf4 v = row_sum(pool[q][j][a]);
            const int f0 = 16 * a + 4 * g;
            if (r == 0 && f0 < pl.d[j + 1]) st4(oq + pl.ooff[j] + f0, v);
          }
        }
      }
    }
  }
}

template <int L, int NT>
__global__ __launch_bounds__(CO_THREADS) void co_action_backward_kernel(
    const float* __restrict__ param, int64_t ld_p, const float* __restrict__ his, int64_t ld_h,
    const float* __restrict__ mask, const float* __restrict__ go, int64_t B, int T, CoPlan pl,
    float* grad_his, float* __restrict__ grad_param) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * CO_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;                                        // (uniform over the wave)
  const float* hb = his + b * T * ld_h;
  const float* mb = mask + b * T;
  const float* gob = go + b * pl.orders * pl.S;
  float* ghb = grad_his + b * T * pl.d[0];
  const int n_sets = pl.indep ? pl.orders : 1, ord_in = pl.indep ? 1 : pl.orders;
  const int ntiles = (T + 15) >> 4, d0 = pl.d[0];

  for (int set = 0; set < n_sets; ++set) {
    const float* ps = param + b * ld_p + (int64_t)set * pl.set_len;
    mf4 f[L][NT][NT], bt[L][NT], wb[L][NT][NT];
    float bu[L][NT];
    load_forward_fragments<L, NT>(ps, pl, r, g, f, bt);
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const int din = pl.d[j], dout = pl.d[j + 1];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const int row = 16 * n + r, c0 = 16 * a + 4 * g;
          wb[j][n][a] = row < din && c0 < dout ? ld4(ps + pl.woff[j] + row * dout + c0)
                                               : splat(0.0f);
        }
      }
#pragma unroll
      for (int a = 0; a < NT; ++a)
        bu[j][a] = pl.bias && 16 * a + r < dout ? gld(ps + pl.boff[j] + 16 * a + r) : 0.0f;
    }
    mf4 gw[L][NT][NT], gb[L][NT];      // gw[j][a][n] in the layout of f[j][a][n]
#pragma unroll
    for (int j = 0; j < L; ++j)
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        gb[j][a] = splat(0.0f);
#pragma unroll
        for (int n = 0; n < NT; ++n) gw[j][a][n] = splat(0.0f);
      }

    for (int tile = 0; tile < ntiles; ++tile) {
      const int t0 = tile * 16, t = t0 + r;
      const float m = t < T ? gld(mb + t) : 0.0f;
      const bool on = m != 0.0f;
      float* ght = ghb + (int64_t)t * d0;
      if (!__any(on)) {                                      // nothing live: zeros, once
        if (set == 0 && t < T) {
#pragma unroll
          for (int n = 0; n < NT; ++n)
            if (16 * n + 4 * g < d0) st4(ght + 16 * n + 4 * g, splat(0.0f));
        }
        continue;
      }
      mf4 x[NT], xu[NT], mu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int tu = t0 + 4 * g + i;
        mu[i] = tu < T ? gld(mb + tu) : 0.0f;
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int f0 = 16 * n + 4 * g, fu = 16 * n + r;
        x[n] = on && f0 < d0 ? ld4(hb + (int64_t)t * ld_h + f0) : splat(0.0f);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          xu[n][i] = mu[i] != 0.0f && fu < d0 ? gld(hb + (int64_t)(t0 + 4 * g + i) * ld_h + fu)
                                              : 0.0f;
      }
      mf4 gh[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) gh[n] = splat(0.0f);

#pragma unroll 1
      for (int q = 0; q < ord_in; ++q) {
        const int p = pl.indep ? set + 1 : q + 1;
        const float* gq = gob + (int64_t)(p - 1) * pl.S;
        // the activations a_0 .. a_(L-1), both layouts (a_L is not needed)
        mf4 at[L][NT], au[L][NT], xm1[NT], um1[NT];
        powers<NT>(x, p, xm1, at[0]);
        powers<NT>(xu, p, um1, au[0]);
#pragma unroll
        for (int j = 0; j + 1 < L; ++j) {
#pragma unroll
          for (int a = 0; a < NT; ++a) {
            mf4 yt = bt[j][a], yu = splat(bu[j][a]);
            if (has<NT>(a, pl.d[j + 1])) {
#pragma unroll
              for (int n = 0; n < NT; ++n) {
                if (has<NT>(n, pl.d[j])) {
#pragma unroll
                  for (int c = 0; c < 4; ++c) {
                    yt = mma(f[j][a][n][c], at[j][n][c], yt);
                    yu = mma(at[j][n][c], f[j][a][n][c], yu);
                  }
                }
              }
              yt = tanh4(yt);
              yu = tanh4(yu);
            }
            at[j + 1][a] = yt;
            au[j + 1][a] = yu;
          }
        }
        // delta'_L, then down the layers
        mf4 dt[NT], du[NT];
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const int f0 = 16 * a + 4 * g, fu = 16 * a + r, dL = pl.d[L];
          dt[a] = (f0 < dL ? ld4(gq + pl.ooff[L - 1] + f0) : splat(0.0f)) * m;
          du[a] = mu * (fu < dL ? gld(gq + pl.ooff[L - 1] + fu) : 0.0f);
        }
#pragma unroll
        for (int j = L - 1; j >= 0; --j) {                  // layer j + 1: d[j] -> d[j + 1]
#pragma unroll
          for (int a = 0; a < NT; ++a) {
            if (has<NT>(a, pl.d[j + 1])) {
              gb[j][a] += dt[a];
#pragma unroll
              for (int n = 0; n < NT; ++n) {
                if (has<NT>(n, pl.d[j])) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) gw[j][a][n] = mma(au[j][n][i], du[a][i], gw[j][a][n]);
                }
              }
            }
          }
          mf4 et[NT], eu[NT];
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            et[n] = eu[n] = splat(0.0f);
            if (j > 0) {
              const int f0 = 16 * n + 4 * g, fu = 16 * n + r, dj = pl.d[j];
              et[n] = (f0 < dj ? ld4(gq + pl.ooff[j - 1] + f0) : splat(0.0f)) * m;
              eu[n] = mu * (fu < dj ? gld(gq + pl.ooff[j - 1] + fu) : 0.0f);
            }
            if (has<NT>(n, pl.d[j])) {
#pragma unroll
              for (int a = 0; a < NT; ++a) {
                if (has<NT>(a, pl.d[j + 1])) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) {
                    et[n] = mma(wb[j][n][a][i], dt[a][i], et[n]);
                    if (j > 0) eu[n] = mma(dt[a][i], wb[j][n][a][i], eu[n]);
                  }
                }
              }
            }
          }
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            if (j > 0) {
              dt[n] = et[n] * (1.0f - at[j][n] * at[j][n]);
              du[n] = eu[n] * (1.0f - au[j][n] * au[j][n]);
            } else {
              gh[n] += (xm1[n] * (float)p) * et[n];
            }
          }
        }
      }

      if (t < T) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int f0 = 16 * n + 4 * g;
          if (f0 < d0) {
            mf4 v = on ? gh[n] : splat(0.0f);
            if (set > 0) v += ld4(ght + f0);                 // this lane's own earlier store
            st4(ght + f0, v);
          }
        }
      }
    }

    float* gp_set = grad_param + b * pl.P + (int64_t)set * pl.set_len;
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const int din = pl.d[j], dout = pl.d[j + 1];
#pragma unroll
      for (int a = 0; a < NT; ++a) {
        const int col = 16 * a + r;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int row = 16 * n + 4 * g + c;
            if (row < din && col < dout) gst(gp_set + pl.woff[j] + row * dout + col, gw[j][a][n][c]);
          }
        }
        if (pl.bias) {
          const mf4 v = row_sum(gb[j][a]);
          const int f0 = 16 * a + 4 * g;
          if (r == 0 && f0 < dout) st4(gp_set + pl.boff[j] + f0, v);
        }
      }
    }
  }
}

// The argument checks of both entries, and the plan.
int co_plan(const char* what, int64_t B, int64_t T, const int* widths, int layers, int orders,
            int bias, int order_indep, int64_t ld_param, int64_t ld_his, CoPlan* pl) {
  DR_REQUIRE(layers >= 1 && layers <= CO_MAX_L, DR_INVALID_ARGUMENT,
             "%s (co_action): %d layers is outside [1, %d]", what, layers, CO_MAX_L);
  DR_REQUIRE(widths != nullptr, DR_INVALID_ARGUMENT, "%s (co_action): widths is null", what);
  for (int j = 0; j <= layers; ++j)
    DR_REQUIRE(widths[j] >= 4 && widths[j] <= CO_MAX_D && widths[j] % 4 == 0, DR_INVALID_ARGUMENT,
               "%s (co_action): width %d is not a multiple of 4 in [4, %d]", what, widths[j],
               CO_MAX_D);
  DR_REQUIRE(orders >= 1 && orders <= CO_MAX_ORDERS, DR_INVALID_ARGUMENT,
             "%s (co_action): orders %d is outside [1, %d]", what, orders, CO_MAX_ORDERS);
  DR_REQUIRE((bias == 0 || bias == 1) && (order_indep == 0 || order_indep == 1),
             DR_INVALID_ARGUMENT, "%s (co_action): bias and order_indep must be 0 or 1", what);
  pl->L = layers;
  pl->orders = orders;
  pl->bias = bias;
  pl->indep = order_indep;
  int off = 0, o = 0;
  for (int j = 0; j <= CO_MAX_L; ++j) pl->d[j] = j <= layers ? widths[j] : 0;
  for (int j = 0; j < CO_MAX_L; ++j) {
    pl->woff[j] = off;
    off += pl->d[j] * pl->d[j + 1];
    pl->boff[j] = off;
    if (bias) off += pl->d[j + 1];
    pl->ooff[j] = o;
    o += pl->d[j + 1];
  }
  pl->set_len = off;
  pl->S = o;
  pl->P = off * (order_indep ? orders : 1);
  DR_REQUIRE(T >= 1, DR_INVALID_ARGUMENT, "%s (co_action): T %lld is below 1", what, (long long)T);
  DR_REQUIRE(ld_param % 4 == 0 && ld_param >= pl->P, DR_INVALID_ARGUMENT,
             "%s (co_action): param stride %lld is not a multiple of 4 that holds a row of %d",
             what, (long long)ld_param, pl->P);
  DR_REQUIRE(ld_his % 4 == 0 && ld_his >= pl->d[0], DR_INVALID_ARGUMENT,
             "%s (co_action): his stride %lld is not a multiple of 4 that holds a row of %d", what,
             (long long)ld_his, pl->d[0]);
  DR_REQUIRE(B >= 0 && (B == 0 || T <= ((int64_t(1) << 31) - 1) / (B * pl->d[0])),
             DR_INVALID_ARGUMENT, "%s (co_action): B T d0 = %lld x %lld x %d is outside [0, 2^31)",
             what, (long long)B, (long long)T, pl->d[0]);
  return DR_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace dr

using namespace dr;

// LAUNCH(L, NT): NT = 16-wide feature blocks a quantity may span
#define DR_CO_DISPATCH(pl, LAUNCH)                               \
  do {                                                           \
    bool wide = false;                                           \
    for (int j = 0; j <= (pl).L; ++j) wide = wide || (pl).d[j] > 16; \
    if ((pl).L == 1 && !wide) LAUNCH(1, 1);                      \
    else if ((pl).L == 1) LAUNCH(1, 2);                          \
    else if ((pl).L == 2 && !wide) LAUNCH(2, 1);                 \
    else if ((pl).L == 2) LAUNCH(2, 2);                          \
    else if (!wide) LAUNCH(3, 1);                                \
    else LAUNCH(3, 2);                                           \
  } while (0)

extern "C" int dr_co_action_forward(const float* param, int64_t ld_param, const float* his,
                                    int64_t ld_his, const float* mask, int64_t B, int64_t T,
                                    const int* widths, int layers, int orders, int bias,
                                    int order_indep, float* out, void* stream) {
  const char* what = "dr_co_action_forward";
  CoPlan pl;
  if (int rc = co_plan(what, B, T, widths, layers, orders, bias, order_indep, ld_param, ld_his, &pl))
    return rc;
  if (B == 0) return DR_OK;
  DR_REQUIRE(param && his && mask && out, DR_INVALID_ARGUMENT,
             "%s (co_action): a required pointer is null", what);
  DR_REQUIRE(aligned16(param) && aligned16(his) && aligned16(out), DR_INVALID_ARGUMENT,
             "%s (co_action): param, his and out must be 16-byte aligned", what);
  const dim3 grid((unsigned)ceil_div(B, CO_WAVES)), block(CO_THREADS);
#define DR_CO_FWD(LL, NN)                                                                       \
  hipLaunchKernelGGL((co_action_forward_kernel<LL, NN>), grid, block, 0, S(stream), param,      \
                     ld_param, his, ld_his, mask, B, (int)T, pl, out)
  DR_CO_DISPATCH(pl, DR_CO_FWD);
#undef DR_CO_FWD
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_co_action_backward(const float* param, int64_t ld_param, const float* his,
                                     int64_t ld_his, const float* mask, const float* grad_out,
                                     int64_t B, int64_t T, const int* widths, int layers,
                                     int orders, int bias, int order_indep, float* grad_his,
                                     float* grad_param, void* stream) {
  const char* what = "dr_co_action_backward";
  CoPlan pl;
  if (int rc = co_plan(what, B, T, widths, layers, orders, bias, order_indep, ld_param, ld_his, &pl))
    return rc;
  if (B == 0) return DR_OK;
  DR_REQUIRE(param && his && mask && grad_out && grad_his && grad_param, DR_INVALID_ARGUMENT,
             "%s (co_action): a required pointer is null", what);
  DR_REQUIRE(aligned16(param) && aligned16(his) && aligned16(grad_out) && aligned16(grad_his) &&
                 aligned16(grad_param),
             DR_INVALID_ARGUMENT,
             "%s (co_action): param, his, grad_out, grad_his and grad_param must be 16-byte "
             "aligned", what);
  const dim3 grid((unsigned)ceil_div(B, CO_WAVES)), block(CO_THREADS);
#define DR_CO_BWD(LL, NN)                                                                       \
  hipLaunchKernelGGL((co_action_backward_kernel<LL, NN>), grid, block, 0, S(stream), param,     \
                     ld_param, his, ld_his, mask, grad_out, B, (int)T, pl, grad_his, grad_param)
  DR_CO_DISPATCH(pl, DR_CO_BWD);
#undef DR_CO_BWD
  DR_LAUNCH_CHECK();
  return DR_OK;
}
