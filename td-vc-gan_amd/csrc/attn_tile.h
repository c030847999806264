// The attention tile shared by tdvc_wavlm_attention (ssl_wavlm.hip, BIAS: the gated relative position bias) and tdvc_whisper_attention
// (asr_whisper.hip, no gate and no bias table): one workgroup per (row, head, 64 queries), keys and values streamed through LDS in
// tiles of 64 with an online softmax (running maximum and sum); plain fp32 FMAs, a fixed order, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace tdvc {

constexpr int AT_TQ = 64, AT_TK = 64, AT_MAXT = 4096;

struct AttnP {
  const float* q; const float* k; const float* v; long bs, ts;
  int T, H;
  const float* gate; const float* bias_rel;
  float* out; long o_bs, o_ts;
};

// 256 threads: query qi = t / 4 of the tile, part = t % 4. A thread scores its query against the keys 4 i + part of a key tile and
// accumulates the output dimensions [part D/4, (part + 1) D/4) over all 64 keys of the tile (the probabilities pass through LDS).
template <int D, bool BIAS>
__global__ __launch_bounds__(256) void attn_tile_kernel(AttnP p) {
  constexpr int DP = D / 4, LD = D + 4;
  __shared__ __attribute__((aligned(16))) float ks[AT_TK * LD];
  __shared__ __attribute__((aligned(16))) float vs[AT_TK * LD];
  __shared__ float ps[AT_TQ * (AT_TK + 1)];
  const int t = threadIdx.x, qi = t >> 2, part = t & 3;
  const int b = blockIdx.z, n = blockIdx.y, tq = blockIdx.x * AT_TQ + qi;
  const bool valid = tq < p.T;
  const long head = b * p.bs + n * D;
  float qr[D];
#pragma unroll
  for (int c = 0; c < D; c += 4) {
    const float4 v4 = valid ? *reinterpret_cast<const float4*>(p.q + head + (long)tq * p.ts + c) : float4{0.f, 0.f, 0.f, 0.f};
    qr[c] = v4.x; qr[c + 1] = v4.y; qr[c + 2] = v4.z; qr[c + 3] = v4.w;
  }
  float g = 0.f;
  const float* br = nullptr;
  if constexpr (BIAS) {
    g = valid ? p.gate[((long)b * p.H + n) * p.T + tq] : 0.f;
    br = p.bias_rel + (long)n * (2 * p.T - 1) + (p.T - 1) - (valid ? tq : 0);      // br[s] = bias_rel[n][s - tq + T - 1]
  }
  float m = -INFINITY, l = 0.f;
  float acc[DP];
#pragma unroll
  for (int jx = 0; jx < DP; ++jx) acc[jx] = 0.f;
  for (int s0 = 0; s0 < p.T; s0 += AT_TK) {
    for (int u = t; u < AT_TK * DP; u += 256) {                             // DP float4 per key
      const int key = u / DP, c = 4 * (u - key * DP);
      float4 k4 = float4{0.f, 0.f, 0.f, 0.f}, v4 = k4;
      if (s0 + key < p.T) {
        k4 = *reinterpret_cast<const float4*>(p.k + head + (long)(s0 + key) * p.ts + c);
        v4 = *reinterpret_cast<const float4*>(p.v + head + (long)(s0 + key) * p.ts + c);
      }
      *reinterpret_cast<float4*>(ks + key * LD + c) = k4;
      *reinterpret_cast<float4*>(vs + key * LD + c) = v4;
    }
    __syncthreads();
    float sc[AT_TK / 4];
    float tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < AT_TK / 4; ++i) {
      const int key = 4 * i + part, s = s0 + key;
      const float* kr = ks + key * LD;
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < D; c += 4) {
        const float4 k4 = *reinterpret_cast<const float4*>(kr + c);
        a = fmaf(qr[c], k4.x, a); a = fmaf(qr[c + 1], k4.y, a); a = fmaf(qr[c + 2], k4.z, a); a = fmaf(qr[c + 3], k4.w, a);
      }
      if (s >= p.T) a = -INFINITY;
      else if (!valid) a = 0.f;
      else if constexpr (BIAS) a = fmaf(g, br[s], a);
      sc[i] = a;
      tm = fmaxf(tm, a);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 1));
    tm = fmaxf(tm, __shfl_xor(tm, 2));
    const float mn = fmaxf(m, tm);                                          // finite: every tile holds at least one key below T
    const float alpha = expf(m - mn);                                       // 0 in the first tile (m = -inf)
    float ls = 0.f;
#pragma unroll
    for (int i = 0; i < AT_TK / 4; ++i) {
      const float pe = expf(sc[i] - mn);                                    // 0 for a key at or past T
      ps[qi * (AT_TK + 1) + 4 * i + part] = pe;
      ls += pe;
    }
    ls += __shfl_xor(ls, 1);
    ls += __shfl_xor(ls, 2);
    l = fmaf(l, alpha, ls);
    m = mn;
    __syncthreads();
#pragma unroll
    for (int jx = 0; jx < DP; ++jx) acc[jx] *= alpha;
    for (int key = 0; key < AT_TK; ++key) {
      const float pv = ps[qi * (AT_TK + 1) + key];
      const float* vr = vs + key * LD + part * DP;
#pragma unroll
      for (int jx = 0; jx < DP; jx += 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(vr + jx);
        acc[jx] = fmaf(pv, v4.x, acc[jx]); acc[jx + 1] = fmaf(pv, v4.y, acc[jx + 1]);
        acc[jx + 2] = fmaf(pv, v4.z, acc[jx + 2]); acc[jx + 3] = fmaf(pv, v4.w, acc[jx + 3]);
      }
    }
    __syncthreads();
  }
  if (!valid) return;
  float* o = p.out + b * p.o_bs + (long)tq * p.o_ts + n * D + part * DP;
#pragma unroll
  for (int jx = 0; jx < DP; jx += 4) *reinterpret_cast<float4*>(o + jx) = float4{acc[jx] / l, acc[jx + 1] / l, acc[jx + 2] / l, acc[jx + 3] / l};
}

// the launch of either form; the caller has checked d in {16, 32, 64} and the grid limits
template <bool BIAS>
static inline void attn_tile_launch(const AttnP& p, int B, int d, hipStream_t st) {
  const dim3 grid((p.T + AT_TQ - 1) / AT_TQ, p.H, B);
  if (d == 16) hipLaunchKernelGGL((attn_tile_kernel<16, BIAS>), grid, dim3(256), 0, st, p);
  else if (d == 32) hipLaunchKernelGGL((attn_tile_kernel<32, BIAS>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((attn_tile_kernel<64, BIAS>), grid, dim3(256), 0, st, p);
}

}  // namespace tdvc
