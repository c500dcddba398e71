// gru.hip -- GRU / attention-gated GRU (AUGRU, VecAttGRUCell) over a padded
// sequence, forward and backward, one launch each.
//
// TF's GRUCell form, the reset gate applied BEFORE the candidate product:
//   [r, u] = sigmoid(xp[0:2H] + h wh_g)        c = tanh(xp[2H:3H] + (r h) wh_c)
//   u' = (1 - att) u                           h_new = u' h + (1 - u') c
// under dynamic_rnn(sequence_length): a step t >= seq_len[b] writes a zero
// output and carries h.  xp = x W_x + b is formed by the caller.
//
// Mapping (VALU): a wave owns GRU_ROWS batch rows for the whole sequence, the
// time loop runs inside the kernel, lane j holds hidden column j of each of
// its rows.  The state weights are staged once per block in LDS as float4
// groups of four k ([k / 4][column] -> {W[k..k+3][column]}), so a lane's
// ds_read_b128 feeds four fmaf of every row and neighbouring lanes read
// neighbouring 16-byte slots; the state vector of a row goes through a
// per-wave LDS buffer and comes back as broadcast float4 reads.  A row's
// products run as one k-ascending fmaf chain that starts from xp, whatever
// rows share its wave: a row's result does not depend on the batch around it.
// Waves never synchronise after the weights are staged.
#include "dr_common.h"

namespace dr {
namespace {

constexpr int GRU_ROWS = 4;     // batch rows per wave
constexpr int GRU_WAVES = 4;    // waves per block (they share the staged weights)
constexpr int GRU_MAX_H = 64;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.0f - 2.0f / (expf(2.0f * x) + 1.0f); }

// One wave writes an LDS vector and reads it back across lanes: the LDS serves
// a wave's accesses in order, so only the compiler has to keep them in order.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void fma4(float& acc, const float4& s, const float4& w) {
  acc = fmaf(s.x, w.x, acc);
  acc = fmaf(s.y, w.y, acc);
  acc = fmaf(s.z, w.z, acc);
  acc = fmaf(s.w, w.w, acc);
}

// LDS bytes of a block: three [H / 4][H] float4 matrices and, per wave, two
// [GRU_ROWS][64] float vectors and a [GRU_ROWS][64] reduction scratch.
inline size_t gru_lds_bytes(int H) {
  return (size_t)3 * H * H * sizeof(float) + (size_t)GRU_WAVES * 3 * GRU_ROWS * 64 * sizeof(float);
}

// m[(k / 4) * H + j].{k % 4} = src[k * ld + col0 + j]  (forward: sum over the
// row index k of the weight) or src[j * ld + col0 + k] (backward: over its
// column index), k, j < H.
__device__ __forceinline__ void stage(float* m, const float* src, int ld, int col0, int H,
                                      bool transpose) {
  for (int i = threadIdx.x; i < H * H; i += blockDim.x) {
    const int k = i / H, j = i - k * H;
    const float v = transpose ? gld(src + (size_t)j * ld + col0 + k)
                              : gld(src + (size_t)k * ld + col0 + j);
    m[((k >> 2) * H + j) * 4 + (k & 3)] = v;
  }
}

template <bool ATT>
__global__ __launch_bounds__(GRU_WAVES * 64) void gru_forward_kernel(
    const float* __restrict__ xp, const float* __restrict__ wh_g, const float* __restrict__ wh_c,
    const int32_t* __restrict__ seq_len, const float* __restrict__ att, int64_t B, int T, int H,
    float* __restrict__ out, float* __restrict__ h_final, float* __restrict__ saved) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* mr = lds;
  float* mu = mr + H * H;
  float* mc = mu + H * H;
  stage(mr, wh_g, 2 * H, 0, H, false);
  stage(mu, wh_g, 2 * H, H, H, false);
  stage(mc, wh_c, H, 0, H, false);
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * GRU_WAVES + wave) * GRU_ROWS;
  if (row0 >= B) return;
  float* hb = mc + H * H + wave * (3 * GRU_ROWS * 64);     // [GRU_ROWS][64] state
  float* rb = hb + GRU_ROWS * 64;                          // [GRU_ROWS][64] r * state
  const bool on = lane < H;
  const int j = on ? lane : H - 1;                         // idle lanes read in range, store nothing
  const int H3 = 3 * H;

  int len[GRU_ROWS];
  int tmax = 0;
#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) {
    int n = 0;
    if (row0 + r < B) {
      n = __builtin_amdgcn_readfirstlane(gld(seq_len + row0 + r));
      n = n < 0 ? 0 : (n > T ? T : n);
    }
    len[r] = n;
    tmax = n > tmax ? n : tmax;
  }

  // The tile of a step is loaded one step ahead, into the other of two
  // register sets (the time loop is unrolled by two): with one set the value
  // loaded for step t + 1 has to be copied at the loop's end, and the copy
  // waits for the load -- a memory round trip in every step.  The loads are
  // unconditional for the same reason (a load under a branch merges with the
  // old value at the branch's end): a row past its length (or past the batch)
  // re-reads its last valid step (row B - 1, step 0), in range, cached, unused.
  struct Tile {
    float xr[GRU_ROWS], xu[GRU_ROWS], xc[GRU_ROWS], at[GRU_ROWS];
  };
  auto fetch = [&](Tile& n, int t) {
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      const int64_t row = row0 + r < B ? row0 + r : B - 1;
      const int last = len[r] > 0 ? len[r] - 1 : 0;
      const size_t p = (size_t)row * T + (t < last ? t : last);
      const float* x = xp + p * H3;
      n.xr[r] = gld(x + j);
      n.xu[r] = gld(x + H + j);
      n.xc[r] = gld(x + 2 * H + j);
      n.at[r] = ATT ? gld(att + p) : 0.0f;
    }
  };
  float h[GRU_ROWS];
#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) {
    h[r] = 0.0f;
    hb[r * 64 + lane] = 0.0f;
  }

  const float4* mr4 = reinterpret_cast<const float4*>(mr);
  const float4* mu4 = reinterpret_cast<const float4*>(mu);
  const float4* mc4 = reinterpret_cast<const float4*>(mc);
  const int HQ = H >> 2;

  auto step = [&](int t, Tile& cur, Tile& nxt) {
    fetch(nxt, t + 1);                   // in flight while this step computes
    __builtin_amdgcn_sched_barrier(0);
    float ar[GRU_ROWS], au[GRU_ROWS], ac[GRU_ROWS];
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      ar[r] = cur.xr[r];
      au[r] = cur.xu[r];
      ac[r] = cur.xc[r];
    }
    for (int kq = 0; kq < HQ; ++kq) {
      const float4 wr = mr4[kq * H + j], wu = mu4[kq * H + j];
#pragma unroll
      for (int r = 0; r < GRU_ROWS; ++r) {
        const float4 hv = *reinterpret_cast<const float4*>(hb + r * 64 + kq * 4);
        fma4(ar[r], hv, wr);
        fma4(au[r], hv, wu);
      }
    }
    float rg[GRU_ROWS], ug[GRU_ROWS];
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      rg[r] = sigmoidf_(ar[r]);
      ug[r] = sigmoidf_(au[r]);
      rb[r * 64 + lane] = rg[r] * h[r];
    }
    wave_sync();
    for (int kq = 0; kq < HQ; ++kq) {
      const float4 wc = mc4[kq * H + j];
#pragma unroll
      for (int r = 0; r < GRU_ROWS; ++r) {
        const float4 hv = *reinterpret_cast<const float4*>(rb + r * 64 + kq * 4);
        fma4(ac[r], hv, wc);
      }
    }
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      if (t < len[r]) {                                    // wave-uniform
        const float c = tanhf_(ac[r]);
        const float up = ATT ? (1.0f - cur.at[r]) * ug[r] : ug[r];
        const float hn = up * h[r] + (1.0f - up) * c;
        h[r] = hn;
        hb[r * 64 + lane] = hn;
        if (on) {
          const size_t p = (size_t)(row0 + r) * T + t;
          gst(out + p * H + lane, hn);
          float* s = saved + p * H3;
          gst(s + lane, rg[r]);
          gst(s + H + lane, ug[r]);
          gst(s + 2 * H + lane, c);
        }
      }
    }
    wave_sync();
  };

  Tile ta, tb;
  fetch(ta, 0);
  for (int t = 0; t < tmax; t += 2) {
    step(t, ta, tb);
    if (t + 1 >= tmax) break;
    step(t + 1, tb, ta);
  }

  // padded steps: zero outputs, zero saved state; the last state of each row
#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) {
    if (row0 + r >= B) continue;
    if (on) gst(h_final + (size_t)(row0 + r) * H + lane, h[r]);
    const size_t base = (size_t)(row0 + r) * T;
    const int n = (T - len[r]) * H;
    float* o = out + (base + len[r]) * H;
    for (int i = lane; i < n; i += 64) gst(o + i, 0.0f);
    float* s = saved + (base + len[r]) * H3;
    for (int i = lane; i < 3 * n; i += 64) gst(s + i, 0.0f);
  }
}

template <bool ATT>
__global__ __launch_bounds__(GRU_WAVES * 64) void gru_backward_kernel(
    const float* __restrict__ wh_g, const float* __restrict__ wh_c,
    const int32_t* __restrict__ seq_len, const float* __restrict__ att,
    const float* __restrict__ out, const float* __restrict__ saved,
    const float* __restrict__ grad_out, const float* __restrict__ grad_h_final, int64_t B, int T,
    int H, float* __restrict__ grad_xp, float* __restrict__ grad_att) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* mr = lds;          // [j / 4][k] -> wh_g[k][j..j+3]       (d pre-r -> d h)
  float* mu = mr + H * H;   //            -> wh_g[k][H + j..]      (d pre-u -> d h)
  float* mc = mu + H * H;   //            -> wh_c[k][j..]          (d pre-c -> d (r h))
  stage(mr, wh_g, 2 * H, 0, H, true);
  stage(mu, wh_g, 2 * H, H, H, true);
  stage(mc, wh_c, H, 0, H, true);
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * GRU_WAVES + wave) * GRU_ROWS;
  if (row0 >= B) return;
  float* pa = mc + H * H + wave * (3 * GRU_ROWS * 64);     // [GRU_ROWS][64] d pre-c, then d pre-r
  float* pb = pa + GRU_ROWS * 64;                          // [GRU_ROWS][64] d pre-u
  float* red = pb + GRU_ROWS * 64;                         // [GRU_ROWS][64] du' * u
  const bool on = lane < H;
  const int j = on ? lane : H - 1;
  const int H3 = 3 * H;

  int len[GRU_ROWS];
  int tmax = 0;
#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) {
    int n = 0;
    if (row0 + r < B) {
      n = __builtin_amdgcn_readfirstlane(gld(seq_len + row0 + r));
      n = n < 0 ? 0 : (n > T ? T : n);
    }
    len[r] = n;
    tmax = n > tmax ? n : tmax;
  }

  // What step t of a row reads: its grad_out, saved gates, h_prev and att,
  // loaded one step ahead into the other of two register sets and
  // unconditionally, as in the forward: step t clamped into the row's valid
  // steps (row B - 1, step 0 for a row past the batch or an empty one).
  struct Tile {
    float go[GRU_ROWS], sr[GRU_ROWS], su[GRU_ROWS], sc[GRU_ROWS], hp[GRU_ROWS], at[GRU_ROWS];
  };
  auto fetch = [&](Tile& n, int t) {
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      const int64_t row = row0 + r < B ? row0 + r : B - 1;
      const int last = len[r] > 0 ? len[r] - 1 : 0;
      const int tc = t < 0 ? 0 : (t < last ? t : last);
      const size_t p = (size_t)row * T + tc;
      n.go[r] = grad_out ? gld(grad_out + p * H + j) : 0.0f;
      const float* s = saved + p * H3;
      n.sr[r] = gld(s + j);
      n.su[r] = gld(s + H + j);
      n.sc[r] = gld(s + 2 * H + j);
      const float prev = gld(out + (p - (tc > 0 ? 1 : 0)) * H + j);
      n.hp[r] = tc > 0 ? prev : 0.0f;
      n.at[r] = ATT ? gld(att + p) : 0.0f;
    }
  };
  float dh[GRU_ROWS];
#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) {
    dh[r] = 0.0f;
    pa[r * 64 + lane] = 0.0f;
    pb[r * 64 + lane] = 0.0f;
    red[r * 64 + lane] = 0.0f;
    if (len[r] > 0 && grad_h_final) dh[r] = gld(grad_h_final + (size_t)(row0 + r) * H + j);
  }

  const float4* mr4 = reinterpret_cast<const float4*>(mr);
  const float4* mu4 = reinterpret_cast<const float4*>(mu);
  const float4* mc4 = reinterpret_cast<const float4*>(mc);
  const int HQ = H >> 2;
  const int rrow = lane >> 4, rseg = lane & 15;            // the att-gradient sum: 16 lanes a row
  int rlen = 0;                                            // the length of that row
  if (row0 + rrow < B) {
    rlen = gld(seq_len + row0 + rrow);
    rlen = rlen < 0 ? 0 : (rlen > T ? T : rlen);
  }

  auto step = [&](int t, Tile& cur, Tile& nxt) {
    fetch(nxt, t - 1);                   // in flight while this step computes
    __builtin_amdgcn_sched_barrier(0);
    const float* rg = cur.sr;
    const float* ug = cur.su;
    const float* c = cur.sc;
    const float* hv = cur.hp;
    const float* a = cur.at;
    float dpc[GRU_ROWS], du[GRU_ROWS], dhp[GRU_ROWS];
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      const bool live = t < len[r];
      const float d = dh[r] + cur.go[r];                   // dh: what later steps passed down
      const float up = ATT ? (1.0f - a[r]) * ug[r] : ug[r];
      const float dc = d * (1.0f - up);
      const float dup = d * (hv[r] - c[r]);
      dhp[r] = d * up;
      du[r] = ATT ? dup * (1.0f - a[r]) : dup;
      dpc[r] = live ? dc * (1.0f - c[r] * c[r]) : 0.0f;
      pa[r * 64 + lane] = on ? dpc[r] : 0.0f;
      if (ATT) red[r * 64 + lane] = (on && live) ? dup * ug[r] : 0.0f;
    }
    wave_sync();
    if (ATT && grad_att) {
      // sum over the columns of row rrow: four strided terms a lane, then an
      // xor tree inside its 16 lanes -- the same order wherever the row sits
      const float* q = red + rrow * 64 + rseg;
      float s = ((q[0] + q[16]) + q[32]) + q[48];
      s += __shfl_xor(s, 8);
      s += __shfl_xor(s, 4);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 1);
      if (rseg == 0 && t < rlen) gst(grad_att + (size_t)(row0 + rrow) * T + t, -s);
    }
    float drh[GRU_ROWS];
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) drh[r] = 0.0f;
    for (int kq = 0; kq < HQ; ++kq) {
      const float4 wc = mc4[kq * H + j];
#pragma unroll
      for (int r = 0; r < GRU_ROWS; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(pa + r * 64 + kq * 4);
        fma4(drh[r], v, wc);
      }
    }
    wave_sync();
    float dpr[GRU_ROWS], dpu[GRU_ROWS];
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      const bool live = t < len[r];
      const float dr = drh[r] * hv[r];
      dhp[r] = dhp[r] + drh[r] * rg[r];
      dpr[r] = live ? dr * rg[r] * (1.0f - rg[r]) : 0.0f;
      dpu[r] = live ? du[r] * ug[r] * (1.0f - ug[r]) : 0.0f;
      pa[r * 64 + lane] = on ? dpr[r] : 0.0f;
      pb[r * 64 + lane] = on ? dpu[r] : 0.0f;
    }
    wave_sync();
    float acc[GRU_ROWS];
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) acc[r] = 0.0f;
    for (int kq = 0; kq < HQ; ++kq) {
      const float4 wr = mr4[kq * H + j], wu = mu4[kq * H + j];
#pragma unroll
      for (int r = 0; r < GRU_ROWS; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(pa + r * 64 + kq * 4);
        const float4 w = *reinterpret_cast<const float4*>(pb + r * 64 + kq * 4);
        fma4(acc[r], v, wr);
        fma4(acc[r], w, wu);
      }
    }
    wave_sync();
#pragma unroll
    for (int r = 0; r < GRU_ROWS; ++r) {
      if (t < len[r]) {                                    // wave-uniform
        dh[r] = dhp[r] + acc[r];
        if (on) {
          float* gx = grad_xp + ((size_t)(row0 + r) * T + t) * H3;
          gst(gx + lane, dpr[r]);
          gst(gx + H + lane, dpu[r]);
          gst(gx + 2 * H + lane, dpc[r]);
        }
      }   // a padded step carries dh (grad_h_final until the row's last valid step)
    }
  };

  Tile ta, tb;
  fetch(ta, tmax - 1);
  for (int t = tmax - 1; t >= 0; t -= 2) {
    step(t, ta, tb);
    if (t == 0) break;
    step(t - 1, tb, ta);
  }

#pragma unroll
  for (int r = 0; r < GRU_ROWS; ++r) {
    if (row0 + r >= B) continue;
    const size_t base = (size_t)(row0 + r) * T + len[r];
    const int n = (T - len[r]) * H3;
    float* gx = grad_xp + base * H3;
    for (int i = lane; i < n; i += 64) gst(gx + i, 0.0f);
    if (ATT && grad_att)
      for (int i = lane; i < T - len[r]; i += 64) gst(grad_att + base + i, 0.0f);
  }
}

int gru_check(const char* what, int64_t B, int64_t T, int64_t H) {
  DR_REQUIRE(H >= 4 && H <= GRU_MAX_H && H % 4 == 0, DR_INVALID_ARGUMENT,
             "%s (gru): hidden %lld has no kernel shape (a multiple of 4 in [4, %d])", what,
             (long long)H, GRU_MAX_H);
  DR_REQUIRE(T >= 1 && T <= (1 << 20), DR_INVALID_ARGUMENT,
             "%s (gru): seq_len %lld is outside [1, 2^20]", what, (long long)T);
  DR_REQUIRE(B >= 0 && B <= (int64_t(1) << 31) - 1, DR_INVALID_ARGUMENT,
             "%s (gru): batch %lld is outside [0, 2^31)", what, (long long)B);
  return DR_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" size_t dr_gru_seq_saved_size(int64_t B, int64_t T, int64_t H) {
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return (size_t)B * (size_t)T * 3 * (size_t)H * sizeof(float);
}

extern "C" int dr_gru_seq_forward(const float* xp, const float* wh_g, const float* wh_c,
                                  const int32_t* seq_len, const float* att, int64_t B, int64_t T,
                                  int64_t H, float* out, float* h_final, float* saved,
                                  void* stream) {
  if (int rc = gru_check("dr_gru_seq_forward", B, T, H)) return rc;
  DR_REQUIRE(xp && wh_g && wh_c && seq_len && out && h_final && saved, DR_INVALID_ARGUMENT,
             "dr_gru_seq_forward (gru): a required pointer is null");
  DR_REQUIRE(aligned16(xp) && aligned16(saved), DR_INVALID_ARGUMENT,
             "dr_gru_seq_forward (gru): the 3H-column blocks xp and saved must be 16-byte aligned");
  if (B == 0) return DR_OK;
  const int64_t tile = GRU_WAVES * GRU_ROWS;
  const dim3 grid((unsigned)ceil_div(B, tile)), block(GRU_WAVES * 64);
  const size_t lds = gru_lds_bytes((int)H);
  if (att)
    hipLaunchKernelGGL(gru_forward_kernel<true>, grid, block, lds, S(stream), xp, wh_g, wh_c,
                       seq_len, att, B, (int)T, (int)H, out, h_final, saved);
  else
    hipLaunchKernelGGL(gru_forward_kernel<false>, grid, block, lds, S(stream), xp, wh_g, wh_c,
                       seq_len, att, B, (int)T, (int)H, out, h_final, saved);
  DR_LAUNCH_CHECK();
  return DR_OK;
}

extern "C" int dr_gru_seq_backward(const float* wh_g, const float* wh_c, const int32_t* seq_len,
                                   const float* att, const float* out, const float* saved,
                                   const float* grad_out, const float* grad_h_final, int64_t B,
                                   int64_t T, int64_t H, float* grad_xp, float* grad_att,
                                   void* stream) {
  if (int rc = gru_check("dr_gru_seq_backward", B, T, H)) return rc;
  DR_REQUIRE(wh_g && wh_c && seq_len && out && saved && grad_xp, DR_INVALID_ARGUMENT,
             "dr_gru_seq_backward (gru): a required pointer is null");
  DR_REQUIRE(!grad_att || att, DR_INVALID_ARGUMENT,
             "dr_gru_seq_backward (gru): grad_att is given without att");
  DR_REQUIRE(aligned16(saved) && aligned16(grad_xp), DR_INVALID_ARGUMENT,
             "dr_gru_seq_backward (gru): the 3H-column blocks saved and grad_xp must be 16-byte "
             "aligned");
  if (B == 0) return DR_OK;
  const int64_t tile = GRU_WAVES * GRU_ROWS;
  const dim3 grid((unsigned)ceil_div(B, tile)), block(GRU_WAVES * 64);
  const size_t lds = gru_lds_bytes((int)H);
  if (att)
    hipLaunchKernelGGL(gru_backward_kernel<true>, grid, block, lds, S(stream), wh_g, wh_c,
                       seq_len, att, out, saved, grad_out, grad_h_final, B, (int)T, (int)H,
                       grad_xp, grad_att);
  else
    hipLaunchKernelGGL(gru_backward_kernel<false>, grid, block, lds, S(stream), wh_g, wh_c,
                       seq_len, att, out, saved, grad_out, grad_h_final, B, (int)T, (int)H,
                       grad_xp, grad_att);
  DR_LAUNCH_CHECK();
  return DR_OK;
}
