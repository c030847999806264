// YIN pitch tracker (util/yin.py:24-140): waveform in, one F0 value per frame out, in ONE launch.
//
// One 256-thread block per (sample, frame). The frame u[0..L), L = 2*tau_max <= 2048 floats, is staged into LDS with the
// reference's zero padding done by index arithmetic. The difference function
//     d[tau] = sum_{j=0}^{L-1-tau} (u[j] - u[j+tau])^2
// is summed directly (the reference's FFT form E + S[L-tau] - S[tau] - 2*corr cancels badly at the minimum). A thread owns
// four consecutive tau (tau0 = 4g) and a slice of j; it walks j four at a time with a sliding register window over
// u[j+tau0 .. j+tau0+7), so two ds_read_b128 (u[j..j+3], the same address in every lane of a slice = broadcast, and the next
// four window values, consecutive 16-byte slots over consecutive lanes = conflict-free) feed 16 subtract-FMA pairs. Rows have
// L - tau terms, so the j range of a row is cut into NC slices of equal length PER ROW: every thread gets the same share of
// its own row, and with several blocks resident per CU the 2:1 spread between the first and the last row evens out.
// Built with -fno-slp-vectorize (csrc/Makefile): packed into v_pk_add/v_pk_fma the loop needs 94 instead of 52 VGPRs and ran 20 % slower.
//
// Accuracy: the test bound is a few fp32 ulps of the CMDF, less than a plain running sum of 2048 terms keeps. Sums run in
// blocks of 16 terms that are folded into the row total with a compensated (Kahan) add: fp32 throughout, +4 VALU per 32.
// Every sum has a fixed order (no atomics): two runs give identical bits.
//
// After the difference function everything stays in LDS: slice fold, prefix sum (4 values per thread, wave64 shuffle scan,
// one cross-wave step), CMDF, and the two searches as block min / sum reductions.
#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include <limits.h>

namespace tdvc {

constexpr int YIN_THREADS = 256;
constexpr int YIN_WAVES = YIN_THREADS / 64;
constexpr int YIN_TAU_CAP = 1024;                 // tau_max the ABI accepts: L = 2048 floats = 8 KiB of LDS
constexpr int YIN_U_FLOATS = 2 * YIN_TAU_CAP + 8; // frame + zeroed tail: the register window reads up to u[L+R+2] (rounded up to 4)
constexpr int YIN_R = 4;                          // consecutive tau per thread
static_assert(YIN_R == 4 || YIN_R == 8, "the zeroed tail covers a window of at most 12 values");
constexpr int YIN_D_FLOATS = YIN_R * YIN_THREADS; // NC slices x (R * NG) rows, NC * NG <= 256

struct YinP {
  const float* x; long x_bs;
  int T, tau_min, tau_max, stride, n_frames;
  int NG, NC;                                     // groups of YIN_R tau; j slices per row
  float threshold, sample_rate; int soft;
  float* f0; float* cmdf;
};

__device__ __forceinline__ int yin_block_min(int v, int* red, int slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[slot * YIN_WAVES + (threadIdx.x >> 6)] = v;
  __syncthreads();
  int r = red[slot * YIN_WAVES];
#pragma unroll
  for (int w = 1; w < YIN_WAVES; ++w) r = min(r, red[slot * YIN_WAVES + w]);
  return r;
}
__device__ __forceinline__ float yin_block_minf(float v, float* red, int slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[slot * YIN_WAVES + (threadIdx.x >> 6)] = v;
  __syncthreads();
  float r = red[slot * YIN_WAVES];
#pragma unroll
  for (int w = 1; w < YIN_WAVES; ++w) r = fminf(r, red[slot * YIN_WAVES + w]);
  return r;
}
__device__ __forceinline__ float yin_block_sum(float v, float* red, int slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // butterfly: the same tree in every lane and every run
  if ((threadIdx.x & 63) == 0) red[slot * YIN_WAVES + (threadIdx.x >> 6)] = v;
  __syncthreads();
  float r = red[slot * YIN_WAVES];
#pragma unroll
  for (int w = 1; w < YIN_WAVES; ++w) r += red[slot * YIN_WAVES + w];
  return r;
}

// acc[r] += (a_i - w[i + r])^2 for the four j of one step; W = the seven window values u[j+tau0 .. j+tau0+6]
#define YIN_STEP(acc, a, W)                                        \
  _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {               \
    _Pragma("unroll") for (int r_ = 0; r_ < YIN_R; ++r_) {        \
      float df_ = a[i_] - W[i_ + r_];                              \
      acc[r_] = fmaf(df_, df_, acc[r_]);                           \
    }                                                              \
  }

__global__ __launch_bounds__(YIN_THREADS) void yin_f0_kernel(YinP p) {
  __shared__ __attribute__((aligned(16))) float u[YIN_U_FLOATS];
  __shared__ __attribute__((aligned(16))) float dpart[YIN_D_FLOATS];
  __shared__ float redf[6 * YIN_WAVES];
  __shared__ int redi[2 * YIN_WAVES];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.n_frames, f = blockIdx.x - b * p.n_frames;
  const int L = 2 * p.tau_max;
  const int Lz = ((L + 3) & ~3) + 8;

  // ---- stage the frame: padded[i] = x[i - L/2] inside [0, T), else 0 (right extension to L and both pads are zeros alike)
  {
    const float* xb = p.x + (long)b * p.x_bs;
    const long s0 = (long)f * p.stride - p.tau_max;
    for (int j = tid; j < Lz; j += YIN_THREADS) {
      long s = s0 + j;
      u[j] = (j < L && s >= 0 && s < p.T) ? xb[s] : 0.f;
    }
  }
  __syncthreads();

  // ---- difference function: thread = (slice c, tau group g)
  const int g = tid % p.NG, c = tid / p.NG;
  if (c < p.NC) {
    constexpr int R = YIN_R;
    const int tau0 = R * g;
    const int Lr = L - tau0;                                   // terms of the group's longest row
    const int ja = ((long)c * Lr / p.NC) & ~3;
    const int jb = (c + 1 == p.NC) ? ((Lr + 3) & ~3) : (int)(((long)(c + 1) * Lr / p.NC) & ~3);
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
      reinterpret_cast<float4*>(dpart)[(c * p.NG + g) * (R / 4) + q] = make_float4(sum[4 * q], sum[4 * q + 1], sum[4 * q + 2], sum[4 * q + 3]);
  }
  __syncthreads();

  // ---- CMDF: c[k] = d[k+1] * (k+1) / max(sum_{i<=k+1} d[i], 1e-5), k = 0 .. tau_max-2; thread owns k = 4*tid .. 4*tid+3
  const int n1 = p.tau_max - 1;
  const int n = n1 - p.tau_min;
  const int rowlen = YIN_R * p.NG;
  float* cl = u;                                                // the frame is dead: its LDS holds the CMDF from here on
  float v[4], pre[4];
  {
    float run = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * tid + e;
      float d = 0.f;
      if (k < n1) {
        d = dpart[k + 1];
        for (int s = 1; s < p.NC; ++s) d += dpart[s * rowlen + k + 1];      // slices in order
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
    if ((tid & 63) == 63) redf[tid >> 6] = incl;
    __syncthreads();
    float base = 0.f;
    for (int w = 0; w < (tid >> 6); ++w) base += redf[w];
    base += incl - run;                                         // everything before this thread's four values
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * tid + e;
      if (k >= p.tau_min && k < n1) {
        float num = v[e] * (float)(k + 1);                      // product first, then the divide
        cl[k - p.tau_min] = num / fmaxf(base + pre[e], 1e-5f);
      }
    }
  }
  __syncthreads();

  const long fr = (long)b * p.n_frames + f;
  if (p.cmdf) {
    float* out = p.cmdf + fr * n;
    for (int k = tid; k < n; k += YIN_THREADS) out[k] = cl[k];
  }

  float tau;
  if (!p.soft) {
    // first index below the threshold (index 0 counts as none), then the first index from there on whose successor is not smaller
    int fb = INT_MAX;
    for (int k = tid; k < n; k += YIN_THREADS)
      if (cl[k] < p.threshold) { fb = k; break; }
    fb = yin_block_min(fb, redi, 0);
    int cand = INT_MAX;
    if (fb != INT_MAX && fb > 0) {
      for (int k = tid; k < n; k += YIN_THREADS)
        if (k >= fb && (k == n - 1 || cl[k + 1] - cl[k] >= 0.f)) { cand = k; break; }
    }
    cand = yin_block_min(cand, redi, 1);
    tau = (cand == INT_MAX) ? 0.f : (float)cand;
  } else {
    // tau = sum_k softmax(-100 c)[k] * k, times 1 if any c is below the threshold
    float mn = INFINITY;
    for (int k = tid; k < n; k += YIN_THREADS) mn = fminf(mn, cl[k]);
    mn = yin_block_minf(mn, redf, 1);
    const float xmax = -mn * 100.f;
    float se = 0.f, sk = 0.f;
    for (int k = tid; k < n; k += YIN_THREADS) {
      float e = expf(-cl[k] * 100.f - xmax);
      se += e;
      sk = fmaf(e, (float)k, sk);
    }
    se = yin_block_sum(se, redf, 2);
    sk = yin_block_sum(sk, redf, 3);
    tau = (mn < p.threshold) ? sk / se : 0.f;
  }
  if (tid == 0) p.f0[fr] = tau > 0.f ? p.sample_rate / ((tau + (float)p.tau_min) + 1.f) : 0.f;
}

}  // namespace tdvc

extern "C" int tdvc_yin_num_frames(int32_t T, int32_t tau_max, int32_t stride) {
  if (T < 1 || tau_max < 1 || stride < 1) return 0;
  const long L = 2L * tau_max;
  return (int)(((T > L ? (long)T : L) - 1) / stride + 1);
}

extern "C" int tdvc_yin_f0(const float* x, int64_t x_bs, int32_t B, int32_t T, int32_t tau_min, int32_t tau_max, int32_t stride,
                           float threshold, int32_t soft, float sample_rate, float* f0, float* cmdf, void* stream) {
  using namespace tdvc;
  if (T < 1) return tdvc_fail(TDVC_EINVAL, "yin_f0: T must be >= 1");
  if (stride < 1) return tdvc_fail(TDVC_EINVAL, "yin_f0: stride must be >= 1");
  if (tau_min < 0 || (long)tau_max - 1 - tau_min < 2) return tdvc_fail(TDVC_EINVAL, "yin_f0: needs 0 <= tau_min and tau_max - 1 - tau_min >= 2");
  if (tau_max > YIN_TAU_CAP) return tdvc_fail(TDVC_EUNSUPPORTED, "yin_f0: tau_max above 1024 (the frame no longer fits the kernel's LDS image)");
  if (B < 1 || x_bs < 0 || !(sample_rate > 0.f)) return tdvc_fail(TDVC_EINVAL, "yin_f0: bad batch, batch stride or sample rate");
  if (!x || !f0) return tdvc_fail(TDVC_EINVAL, "yin_f0: null pointer");
  const int nf = tdvc_yin_num_frames(T, tau_max, stride);
  if ((long)B * nf > INT_MAX) return tdvc_fail(TDVC_EUNSUPPORTED, "yin_f0: more than 2^31-1 frames in one call");
  YinP p;
  p.x = x; p.x_bs = x_bs; p.T = T; p.tau_min = tau_min; p.tau_max = tau_max; p.stride = stride; p.n_frames = nf;
  p.NG = (tau_max + YIN_R - 1) / YIN_R;
  p.NC = YIN_THREADS / p.NG;                                   // NG <= 256, so NC >= 1 and NC * NG <= 256
  p.threshold = threshold; p.sample_rate = sample_rate; p.soft = soft ? 1 : 0;
  p.f0 = f0; p.cmdf = cmdf;
  auto k = yin_f0_kernel;
  TDVC_TRACE(k);
  hipLaunchKernelGGL(k, dim3(B * nf), dim3(YIN_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
