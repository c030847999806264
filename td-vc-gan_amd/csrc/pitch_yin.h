// Device code the YIN forward (pitch_yin.hip) and the soft-YIN backward (pitch_yin_bwd.hip) both run: frame staging, the
// difference function, the CMDF and the softmax search. The backward RECOMPUTES the forward's intermediates with these very
// functions, so its tau / f0 carry the forward's bits. Layout and accuracy notes: pitch_yin.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include "reduce.h"

namespace tdvc {

constexpr int YIN_THREADS = 256;
constexpr int YIN_WAVES = YIN_THREADS / 64;
constexpr int YIN_TAU_CAP = 1024;                 // tau_max the ABI accepts: L = 2048 floats = 8 KiB of LDS
constexpr int YIN_U_FLOATS = 2 * YIN_TAU_CAP + 8; // frame + zeroed tail: the register window reads up to u[L+R+2] (rounded up to 4)
constexpr int YIN_R = 4;                          // consecutive tau per thread
static_assert(YIN_R == 4 || YIN_R == 8, "the zeroed tail covers a window of at most 12 values");
constexpr int YIN_D_FLOATS = YIN_R * YIN_THREADS; // NC slices x (R * NG) rows, NC * NG <= 256
constexpr int YIN_RED_SLOTS = 6;                  // block-reduction slots of YIN_WAVES values each
constexpr float YIN_FLOOR = 1e-5f;                // floor of the CMDF's denominator

// the block reductions of reduce.h on slot `slot` of red (a slot per reduction: no barrier protects a reuse); the sum adds the wave
// values left to right
template <typename T>
__device__ __forceinline__ T yin_block_min(T v, T* red, int slot) { return block_min<YIN_WAVES>(v, red + slot * YIN_WAVES, threadIdx.x); }
__device__ __forceinline__ float yin_block_sum(float v, float* red, int slot) {
  return block_sum_in_order<YIN_WAVES>(v, red + slot * YIN_WAVES, threadIdx.x);
}

// acc[r] += (a_i - w[i + r])^2 for the four j of one step; W = the seven window values u[j+tau0 .. j+tau0+6]
#define YIN_STEP(acc, a, W)                                        \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {               \
    _Pragma("unroll") for (int r_ = 0; r_ < YIN_R; ++r_) {        \
      float df_ = a[i_] - W[i_ + r_];                              \
      acc[r_] = fmaf(df_, df_, acc[r_]);                           \
    }                                                              \
  }

// ---- stage the frame: padded[i] = x[i - L/2] inside [0, T), else 0 (right extension to L and both pads are zeros alike).
// Writes u[0 .. roundup4(L) + 8); the caller synchronises.
__device__ __forceinline__ void yin_stage_frame(const float* x, long x_bs, int T, int tau_max, int stride, int b, int f, float* u) {
  const int tid = threadIdx.x;
  const int L = 2 * tau_max;
  const int Lz = ((L + 3) & ~3) + 8;
  const float* xb = x + (long)b * x_bs;
  const long s0 = (long)f * stride - tau_max;
  for (int j = tid; j < Lz; j += YIN_THREADS) {
    long s = s0 + j;
    u[j] = (j < L && s >= 0 && s < T) ? xb[s] : 0.f;
  }
}

// ---- difference function: thread = (slice c, tau group g); dpart[c][R * NG] receives the slice sums. The caller synchronises.
__device__ __forceinline__ void yin_difference(const float* u, float* dpart, int L, int NG, int NC) {
  const int tid = threadIdx.x;
  const int g = tid % NG, c = tid / NG;
  if (c < NC) {
    constexpr int R = YIN_R;
    const int tau0 = R * g;
    const int Lr = L - tau0;                                   // terms of the group's longest row
    const int ja = ((long)c * Lr / NC) & ~3;
    const int jb = (c + 1 == NC) ? ((Lr + 3) & ~3) : (int)(((long)(c + 1) * Lr / NC) & ~3);
    const int jfast = min(jb, (L - (R + 2) - tau0) & ~3);      // steps j < jfast have all 4 * R terms inside their rows
    const float4* u4 = reinterpret_cast<const float4*>(u);
    float sum[R], comp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) sum[r] = comp[r] = 0.f;
    float W[R + 4];                                            // u[j+tau0 .. j+tau0+R+3]: R held, four read per step
    int j = ja;
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
      float4 w0 = u4[((j + tau0) >> 2) + q];
      W[4 * q] = w0.x; W[4 * q + 1] = w0.y; W[4 * q + 2] = w0.z; W[4 * q + 3] = w0.w;
    }
    while (j < jb) {
      float blk[R];
#pragma unroll
      for (int r = 0; r < R; ++r) blk[r] = 0.f;
      if (j + 16 <= jfast) {
#pragma unroll
        for (int s = 0; s < 4; ++s, j += 4) {
          float4 av = u4[j >> 2], wn = u4[((j + tau0) >> 2) + R / 4];
          float a[4] = {av.x, av.y, av.z, av.w};
          W[R] = wn.x; W[R + 1] = wn.y; W[R + 2] = wn.z; W[R + 3] = wn.w;
          YIN_STEP(blk, a, W);
#pragma unroll
          for (int q = 0; q < R; ++q) W[q] = W[q + 4];
        }
      } else {                                                 // the row ends: at most one short block, terms masked by row length
        for (int s = 0; s < 4 && j < jb; ++s, j += 4) {
          float4 av = u4[j >> 2], wn = u4[((j + tau0) >> 2) + R / 4];
          float a[4] = {av.x, av.y, av.z, av.w};
          W[R] = wn.x; W[R + 1] = wn.y; W[R + 2] = wn.z; W[R + 3] = wn.w;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
              float df = (j + i + tau0 + r < L) ? a[i] - W[i + r] : 0.f;
              blk[r] = fmaf(df, df, blk[r]);
            }
          }
#pragma unroll
          for (int q = 0; q < R; ++q) W[q] = W[q + 4];
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {                            // compensated add of the block sum
        float y = blk[r] - comp[r];
        float t = sum[r] + y;
        comp[r] = (t - sum[r]) - y;
        sum[r] = t;
      }
    }
#pragma unroll
    for (int q = 0; q < R / 4; ++q)
      reinterpret_cast<float4*>(dpart)[(c * NG + g) * (R / 4) + q] = make_float4(sum[4 * q], sum[4 * q + 1], sum[4 * q + 2], sum[4 * q + 3]);
  }
}

// ---- CMDF: c[k] = d[k+1] * (k+1) / max(sum_{i<=k+1} d[i], 1e-5), k = 0 .. tau_max-2; thread owns k = 4*tid .. 4*tid+3.
// cl[k - tau_min] receives c[k] for k >= tau_min; d[e] and S[e] return the thread's own d[k+1] and running sums (zero and
// the total beyond the last k). Uses red[0 .. YIN_WAVES) and synchronises once inside; the caller synchronises after.
__device__ __forceinline__ void yin_cmdf(const float* dpart, float* red, float* cl, int tau_min, int tau_max, int NG, int NC,
                                         float (&v)[4], float (&S)[4]) {
  const int tid = threadIdx.x;
  const int n1 = tau_max - 1;
  const int rowlen = YIN_R * NG;
  float pre[4];
  float run = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * tid + e;
    float d = 0.f;
    if (k < n1) {
      d = dpart[k + 1];
      for (int s = 1; s < NC; ++s) d += dpart[s * rowlen + k + 1];      // slices in order
    }
    v[e] = d;
    run += d;
    pre[e] = run;
  }
  float incl = run;                                           // wave64 inclusive scan of the thread totals
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float t = __shfl_up(incl, o, 64);
    if ((tid & 63) >= o) incl += t;
  }
  if ((tid & 63) == 63) red[tid >> 6] = incl;
  __syncthreads();
  float base = 0.f;
  for (int w = 0; w < (tid >> 6); ++w) base += red[w];
  base += incl - run;                                         // everything before this thread's four values
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * tid + e;
    S[e] = base + pre[e];
    if (k >= tau_min && k < n1) {
      float num = v[e] * (float)(k + 1);                      // product first, then the divide
      cl[k - tau_min] = num / fmaxf(S[e], YIN_FLOOR);
    }
  }
}

// Unnormalised softmax weight of a CMDF entry c against the minimum mn: exp(100 (mn - c)). The difference comes first, so the
// minimum itself weighs exactly 1: a frame whose other weights vanish then has se = 1 and sk = k* exactly, tau = k*, and the
// backward's (k* - tau) is 0. Written as exp(-100 c + 100 mn) the compiler contracts -100 c + const into an FMA, the argument at the
// minimum is the rounding error of 100 mn instead of 0, and fl(fl(k* e) / e) can land one ulp off k*: times g_tau * 100 that ulp
// was the whole gradient of a saturated frame. The forward and the backward both take their weights from here.
__device__ __forceinline__ float yin_soft_weight(float c, float mn) { return expf((mn - c) * 100.f); }

// ---- soft search over cl[0 .. n): mn = min c, se = sum_k exp(100 (mn - c[k])), sk = sum_k exp(..) * k, so that
// tau = sk / se where mn is below the threshold. Uses red slots 1..3.
__device__ __forceinline__ void yin_soft_search(const float* cl, int n, float* red, float& mn, float& se, float& sk) {
  const int tid = threadIdx.x;
  mn = INFINITY;
  for (int k = tid; k < n; k += YIN_THREADS) mn = fminf(mn, cl[k]);
  mn = yin_block_min(mn, red, 1);
  se = 0.f; sk = 0.f;
  for (int k = tid; k < n; k += YIN_THREADS) {
    float e = yin_soft_weight(cl[k], mn);
    se += e;
    sk = fmaf(e, (float)k, sk);
  }
  se = yin_block_sum(se, red, 2);
  sk = yin_block_sum(sk, red, 3);
}

__device__ __forceinline__ float yin_f0_of_tau(float tau, int tau_min, float sample_rate) {
  return tau > 0.f ? sample_rate / ((tau + (float)tau_min) + 1.f) : 0.f;
}

}  // namespace tdvc
