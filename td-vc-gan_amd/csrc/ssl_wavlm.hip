// The WavLM feature extractor (the reference's wavlm/WavLM.py extract_features in eval mode, restated in include/tdvc.h): the
// layer-norm convolutional front end, the weight-normed grouped positional convolution and the pre-norm transformer encoder with the
// gated relative position bias. Activations are token-major fp32 [B][T][C]; a workgroup sees one row only, so a row's result does not
// depend on its batch. No atomics, fixed summation orders, no host synchronisation.
//
// tdvc_wavlm_gemm       y[b][t][:] = epilogue(A_row(b, t) W^T + bias) on v_mfma_f32_16x16x4_f32 (exact fp32), below
// tdvc_wavlm_conv0      the first convolution (one input channel) with its LayerNorm and GELU, a wave per token, float64 inside
// tdvc_wavlm_layernorm  rows of C floats, a wave per row, float64 statistics; optional GELU; optionally the gates of the relative
//                       position bias from the normalised row (a second tiny launch, float64 inside)
// tdvc_wavlm_posconv    the grouped positional convolution + GELU + residual: the GEMM in its segmented-row mode, a group per
//                       blockIdx.z slice
// tdvc_wavlm_attention  one workgroup per (row, head, 64 queries): keys and values streamed through LDS in tiles of 64 with an online
//                       softmax (running maximum and sum), the gated bias read from the bias_rel table; plain fp32 FMAs (attn_tile.h)
//
// The GEMM. A workgroup of 256 threads (4 waves) owns 64 tokens (32 where 64 would give fewer than 512 workgroups) x 64 output columns; wave w owns the columns [16 w, 16 w + 16) as four
// 16 x 16 accumulator tiles over the tokens (four independent MFMA chains, as in tdvc_tdnn_fwd). The MFMA's M index is the output
// column, so a lane ends with four CONSECUTIVE columns of one token and stores them as one float4 into the token-major output. The
// reduction runs over chunks of 32: the A rows and the weight rows are staged k-contiguous in LDS with a row pitch of 36 floats, each
// lane reads one float4 (four consecutive k) per operand tile and issues four MFMAs from it; which k a lane's q-th slot carries is the
// same for both operands, and the order is fixed. The next chunk is loaded into registers before the MFMAs of this one. Every chunk is
// summed from zero and then added to the running sum (blocked summation: the rounding of K = 4096 or 8192 stays that of 32 + K / 32
// terms). An A row is K contiguous floats, or K / seg_len segments of seg_len floats a fixed stride apart (the taps of the grouped
// positional convolution in the zero-padded token-major buffer).
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "attn_tile.h"
#include "reduce.h"

namespace tdvc {

constexpr int GM_TN = 64, GM_KC = 32, GM_LD = 36, GM_THREADS = 256;
constexpr int WL_MAXC = 1024;       // conv0 / layernorm: 16 values per lane

typedef float wl_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wl_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ double wl_gelu(double v) { return 0.5 * v * (1.0 + erf(v * 0.70710678118654752440)); }

// ------------------------------------------------------------------------------------------------------------------- GEMM
struct GemmP {
  int T, N, K, groups, seg_len, gelu, scale_lo, scale_hi;
  float scale;
  const float* x; long x_bs, x_ts, x_ss, x_gs;
  const float* w; const float* bias;
  const float* res; long r_bs, r_ts;
  float* y; long y_bs, y_ts;
};

template <int NT>                                                           // 16 NT tokens per workgroup: 64, or 32 where 64 would leave CUs idle
__global__ __launch_bounds__(GM_THREADS, 2) void wavlm_gemm_kernel(GemmP p) {
  constexpr int GM_TT = 16 * NT, XS = NT / 2;                               // XS float4 of the A tile per thread
  __shared__ __attribute__((aligned(16))) float xs[GM_TT * GM_LD];
  __shared__ __attribute__((aligned(16))) float ws[GM_TN * GM_LD];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = lane & 15, q = lane >> 4;
  const int b = blockIdx.z / p.groups, g = blockIdx.z - b * p.groups;
  const int t0 = blockIdx.x * GM_TT, n0 = blockIdx.y * GM_TN;
  const bool live = n0 + 16 * w < p.N;                                      // wave-uniform; N is a multiple of 16
  const float* xb = p.x + b * p.x_bs + g * p.x_gs;
  const float* wb = p.w + (long)g * p.N * p.K;
  // staging: float4 u = t + 256 sl of a 64 x 32 tile is row u / 8, columns 4 (u % 8) .. + 3; 256 % 8 == 0: one column per thread
  const int col = 4 * (t & 7);
  const float* xrow[XS];
  const float* wrow[2];
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const int r = (t + GM_THREADS * sl) >> 3;
    if (sl < XS) xrow[sl] = t0 + r < p.T ? xb + (long)(t0 + r) * p.x_ts : nullptr;
    wrow[sl] = n0 + r < p.N ? wb + (long)(n0 + r) * p.K : nullptr;
  }
  float4 xreg[XS], wreg[2];
  auto load = [&](int c0) {
    const int kk = c0 + col;                                                // K and seg_len are multiples of 16: a float4 stays inside
    const bool in = kk < p.K;
    long xo = kk;
    if (p.seg_len) {
      const int s = kk / p.seg_len;
      xo = (long)s * p.x_ss + (kk - s * p.seg_len);
    }
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      if (sl < XS) xreg[sl] = in && xrow[sl] ? *reinterpret_cast<const float4*>(xrow[sl] + xo) : float4{0.f, 0.f, 0.f, 0.f};
      wreg[sl] = in && wrow[sl] ? *reinterpret_cast<const float4*>(wrow[sl] + kk) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  wl_f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = wl_f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int c0 = 0; c0 < p.K; c0 += GM_KC) {
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const int r = (t + GM_THREADS * sl) >> 3;
      if (sl < XS) *reinterpret_cast<float4*>(xs + r * GM_LD + col) = xreg[sl];
      *reinterpret_cast<float4*>(ws + r * GM_LD + col) = wreg[sl];
    }
    __syncthreads();
    if (c0 + GM_KC < p.K) load(c0 + GM_KC);
    if (live) {
      wl_f32x4 part[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) part[nt] = wl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < GM_KC / 16; ++h) {
        const float4 a = *reinterpret_cast<const float4*>(ws + (16 * w + j) * GM_LD + h * 16 + q * 4);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const float4 v = *reinterpret_cast<const float4*>(xs + (nt * 16 + j) * GM_LD + h * 16 + q * 4);
          part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, v.x, part[nt], 0, 0, 0);
          part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, v.y, part[nt], 0, 0, 0);
          part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, v.z, part[nt], 0, 0, 0);
          part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, v.w, part[nt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] += part[nt];
    }
    __syncthreads();
  }
  if (!live) return;
  const int n = g * p.N + n0 + 16 * w + 4 * q;                              // this lane's four columns n .. n + 3
  float add[4], mul[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    add[r] = p.bias ? p.bias[n + r] : 0.f;
    mul[r] = n + r >= p.scale_lo && n + r < p.scale_hi ? p.scale : 1.f;
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int tt = t0 + nt * 16 + j;
    if (tt >= p.T) continue;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = (acc[nt][r] + add[r]) * mul[r];
      if (p.gelu) v[r] = wl_gelu(v[r]);
    }
    if (p.res) {
      const float4 rr = *reinterpret_cast<const float4*>(p.res + b * p.r_bs + tt * p.r_ts + n);
      v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
    }
    *reinterpret_cast<float4*>(p.y + b * p.y_bs + tt * p.y_ts + n) = float4{v[0], v[1], v[2], v[3]};
  }
}

static int gemm_check(const tdvc_wavlm_gemm_args* a, const char** why) {
  *why = nullptr;
  if (!a) { *why = "wavlm_gemm: null arguments"; return TDVC_EINVAL; }
  if (a->B < 0 || a->T < 0 || a->N < 1 || a->K < 1 || a->groups < 1 || a->seg_len < 0 || a->x_bs < 0 || a->x_ts < 0 || a->x_ss < 0 || a->x_gs < 0 ||
      a->r_bs < 0 || a->r_ts < 0 || a->y_bs < 0 || a->y_ts < 0) { *why = "wavlm_gemm: negative size or stride"; return TDVC_EINVAL; }
  if (a->epilogue < 0 || a->epilogue > 1) { *why = "wavlm_gemm: epilogue must be 0 (none) or 1 (erf-GELU)"; return TDVC_EINVAL; }
  if (a->N % 16 || a->K % 16 || a->seg_len % 16) { *why = "wavlm_gemm: N, K and seg_len must be multiples of 16"; return TDVC_EUNSUPPORTED; }
  if (a->seg_len && a->K % a->seg_len) { *why = "wavlm_gemm: K must be a multiple of seg_len"; return TDVC_EINVAL; }
  if ((long)a->B * a->groups > 65535 || a->N > (1 << 20) || a->K > (1 << 24) || a->T > (1 << 24)) {
    *why = "wavlm_gemm: B x groups > 65535, N > 2^20, K or T > 2^24"; return TDVC_EUNSUPPORTED;
  }
  if ((a->x_bs | a->x_ts | a->x_ss | a->x_gs | a->r_bs | a->r_ts | a->y_bs | a->y_ts) & 3) { *why = "wavlm_gemm: strides must be multiples of 4 floats"; return TDVC_EINVAL; }
  if (a->y_ts < (int64_t)a->groups * a->N) { *why = "wavlm_gemm: output token stride below groups x N"; return TDVC_EINVAL; }
  if ((((uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->res | (uintptr_t)a->y) & 15) != 0) { *why = "wavlm_gemm: x, w, residual and y must be 16-byte aligned"; return TDVC_EINVAL; }
  if (a->res && a->res == a->y && (a->r_bs != a->y_bs || a->r_ts != a->y_ts)) { *why = "wavlm_gemm: a residual that is y must have y's strides"; return TDVC_EINVAL; }
  if (a->B == 0 || a->T == 0) return TDVC_OK;
  if (!a->x || !a->w || !a->y) { *why = "wavlm_gemm: null pointer"; return TDVC_EINVAL; }
  return TDVC_OK;
}

static void gemm_launch(const tdvc_wavlm_gemm_args* a, hipStream_t st) {
  GemmP p;
  p.T = a->T; p.N = a->N; p.K = a->K; p.groups = a->groups; p.seg_len = a->seg_len == a->K ? 0 : a->seg_len; p.gelu = a->epilogue;
  p.scale_lo = a->scale_lo; p.scale_hi = a->scale_hi; p.scale = a->scale;
  p.x = a->x; p.x_bs = a->x_bs; p.x_ts = a->x_ts; p.x_ss = a->x_ss; p.x_gs = a->x_gs; p.w = a->w; p.bias = a->bias;
  p.res = a->res; p.r_bs = a->r_bs; p.r_ts = a->r_ts; p.y = a->y; p.y_bs = a->y_bs; p.y_ts = a->y_ts;
  // fewer than 512 workgroups of 64 tokens (two per CU of 256): halve the token tile. An element's summation order is the same in both.
  const long cols = (a->N + GM_TN - 1) / GM_TN, z = (long)a->B * a->groups;
  if ((long)((a->T + 63) / 64) * cols * z < 512)
    hipLaunchKernelGGL(wavlm_gemm_kernel<2>, dim3((a->T + 31) / 32, cols, z), dim3(GM_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL(wavlm_gemm_kernel<4>, dim3((a->T + 63) / 64, cols, z), dim3(GM_THREADS), 0, st, p);
}

// ------------------------------------------------------------------------------------------------------- conv0, LayerNorm
struct NormP {
  const float* x; long x_bs, x_ts;
  int T, C, K, gelu;                // K > 0: x is the waveform row, x_ts its stride in samples, wt [K][C]
  const float* wt; const float* gamma; const float* beta;
  float* y; long y_bs, y_ts;
};

// a wave per token; channel c = lane + 64 i. The row is a K-tap convolution of the waveform (K > 0) or is read.
__global__ __launch_bounds__(256) void wavlm_norm_kernel(NormP p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  {
    const int tt = blockIdx.x * 4 + w;
    if (tt >= p.T) return;                                                  // wave-uniform
    const float* xr = p.x + b * p.x_bs + (long)tt * p.x_ts;
    double v[WL_MAXC / 64];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < WL_MAXC / 64; ++i) {
      const int c = lane + 64 * i;
      double a = 0.0;
      if (c < p.C) {
        if (p.K > 0) {
          for (int k = 0; k < p.K; ++k) a = fma((double)xr[k], (double)p.wt[k * p.C + c], a);
        } else {
          a = (double)xr[c];
        }
      }
      v[i] = a;
      s += a;
    }
    const double mean = wave_sum(s) / (double)p.C;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < WL_MAXC / 64; ++i) {
      const double dlt = lane + 64 * i < p.C ? v[i] - mean : 0.0;
      ss = fma(dlt, dlt, ss);
    }
    const double rstd = 1.0 / sqrt(wave_sum(ss) / (double)p.C + 1e-5);
    float* yr = p.y + b * p.y_bs + (long)tt * p.y_ts;
#pragma unroll
    for (int i = 0; i < WL_MAXC / 64; ++i) {
      const int c = lane + 64 * i;
      if (c >= p.C) continue;
      double o = (v[i] - mean) * rstd * (double)p.gamma[c] + (double)p.beta[c];
      if (p.gelu) o = wl_gelu(o);
      yr[c] = (float)o;
    }
  }
}

// gate[b][n][t] = a (b' grep_a[n] - 1) + 2, a = sigmoid(u0 + .. + u3), b' = sigmoid(u4 + .. + u7), u = grep_w h[t, n d : (n + 1) d] + grep_b
__global__ __launch_bounds__(256) void wavlm_gate_kernel(const float* h, long h_bs, long h_ts, int T, int H, int d, const float* gw, const float* gb,
                                                         const float* ga, float* gate) {
  const long idx = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;               // eight lanes per (token, head): lane `sub` takes c = sub + 8 i
  const int b = blockIdx.y, sub = threadIdx.x & 7;
  if (idx >= (long)T * H) return;                                           // uniform over the eight lanes
  const int tt = (int)(idx / H), n = (int)(idx - (long)tt * H);
  const float* hr = h + b * h_bs + (long)tt * h_ts + n * d;
  double u[8];
#pragma unroll
  for (int jx = 0; jx < 8; ++jx) u[jx] = 0.0;
  for (int c = sub; c < d; c += 8) {
    const double hv = (double)hr[c];
#pragma unroll
    for (int jx = 0; jx < 8; ++jx) u[jx] = fma(hv, (double)gw[jx * d + c], u[jx]);
  }
#pragma unroll
  for (int jx = 0; jx < 8; ++jx) {
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) u[jx] += __shfl_xor(u[jx], off);
    u[jx] += (double)gb[jx];
  }
  if (sub) return;
  const double a = 1.0 / (1.0 + exp(-(((u[0] + u[1]) + u[2]) + u[3])));
  const double bb = 1.0 / (1.0 + exp(-(((u[4] + u[5]) + u[6]) + u[7])));
  gate[((long)b * H + n) * T + tt] = (float)(a * (bb * (double)ga[n] - 1.0) + 2.0);
}

}  // namespace tdvc

extern "C" int tdvc_wavlm_gemm(const tdvc_wavlm_gemm_args* a, void* stream) {
  using namespace tdvc;
  const char* why;
  const int rc = gemm_check(a, &why);
  if (rc != TDVC_OK) return tdvc_fail(rc, why);
  if (a->B == 0 || a->T == 0) return TDVC_OK;
  gemm_launch(a, (hipStream_t)stream);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int32_t tdvc_wavlm_frames(int64_t L, int32_t n_layers, const int32_t* kernels, const int32_t* strides) {
  if (L < 0 || n_layers < 1 || !kernels || !strides) return -1;
  for (int i = 0; i < n_layers; ++i) {
    if (kernels[i] < 1 || strides[i] < 1) return -1;
    L = L < kernels[i] ? 0 : (L - kernels[i]) / strides[i] + 1;
  }
  return L > 0x7fffffffLL ? -1 : (int32_t)L;
}

extern "C" int tdvc_wavlm_conv0(const float* x, int64_t x_bs, int32_t B, int32_t L, const float* w_t, int32_t K, int32_t stride, int32_t C,
                                const float* gamma, const float* beta, float* y, int64_t y_bs, int64_t y_ts, void* stream) {
  using namespace tdvc;
  if (B < 0 || L < 0 || K < 1 || stride < 1 || C < 1 || x_bs < 0 || y_bs < 0 || y_ts < 0) return tdvc_fail(TDVC_EINVAL, "wavlm_conv0: negative size or stride");
  if (C % 16 || C > WL_MAXC) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_conv0: C must be a multiple of 16 up to 1024");
  if (K > 64 || B > 65535 || L > (1 << 28)) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_conv0: K > 64, B > 65535 or L > 2^28");
  if (L < K) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_conv0: a row shorter than the kernel has no frame");
  if (y_ts < C) return tdvc_fail(TDVC_EINVAL, "wavlm_conv0: output token stride below C");
  if (B == 0) return TDVC_OK;
  if (!x || !w_t || !gamma || !beta || !y) return tdvc_fail(TDVC_EINVAL, "wavlm_conv0: null pointer");
  NormP p;
  p.x = x; p.x_bs = x_bs; p.x_ts = stride; p.T = (L - K) / stride + 1; p.C = C; p.K = K; p.gelu = 1; p.wt = w_t; p.gamma = gamma; p.beta = beta;
  p.y = y; p.y_bs = y_bs; p.y_ts = y_ts;
  hipLaunchKernelGGL(wavlm_norm_kernel, dim3((p.T + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_wavlm_layernorm(const float* x, int64_t x_bs, int64_t x_ts, int32_t B, int32_t T, int32_t C, const float* gamma, const float* beta,
                                    int32_t gelu, float* y, int64_t y_bs, int64_t y_ts, int32_t H, const float* grep_w, const float* grep_b,
                                    const float* grep_a, float* gate, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || C < 1 || H < 0 || x_bs < 0 || x_ts < 0 || y_bs < 0 || y_ts < 0) return tdvc_fail(TDVC_EINVAL, "wavlm_layernorm: negative size or stride");
  if (gelu < 0 || gelu > 1) return tdvc_fail(TDVC_EINVAL, "wavlm_layernorm: gelu must be 0 or 1");
  if (C % 16 || C > WL_MAXC) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_layernorm: C must be a multiple of 16 up to 1024");
  if (B > 65535 || T > (1 << 24)) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_layernorm: B > 65535 or T > 2^24");
  if (x_ts < C || y_ts < C) return tdvc_fail(TDVC_EINVAL, "wavlm_layernorm: token stride below C");
  if (H > 0 && (C % H || gelu)) return tdvc_fail(TDVC_EINVAL, "wavlm_layernorm: gates need C divisible by H and no GELU");
  if (B == 0 || T == 0) return TDVC_OK;
  if (!x || !gamma || !beta || !y || (H > 0 && (!grep_w || !grep_b || !grep_a || !gate))) return tdvc_fail(TDVC_EINVAL, "wavlm_layernorm: null pointer");
  NormP p;
  p.x = x; p.x_bs = x_bs; p.x_ts = x_ts; p.T = T; p.C = C; p.K = 0; p.gelu = gelu; p.wt = nullptr; p.gamma = gamma; p.beta = beta;
  p.y = y; p.y_bs = y_bs; p.y_ts = y_ts;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wavlm_norm_kernel, dim3((T + 3) / 4, B), dim3(256), 0, st, p);
  if (H > 0)
    hipLaunchKernelGGL(wavlm_gate_kernel, dim3((unsigned)(((long)T * H * 8 + 255) / 256), B), dim3(256), 0, st, (const float*)y, (long)y_bs, (long)y_ts, T, H,
                       C / H, grep_w, grep_b, grep_a, gate);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_wavlm_posconv(const float* xp, int64_t xp_bs, int32_t B, int32_t T, int32_t C, int32_t K, int32_t groups, const float* w,
                                  const float* bias, float* y, int64_t y_bs, int64_t y_ts, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || C < 1 || K < 2 || groups < 1 || xp_bs < 0) return tdvc_fail(TDVC_EINVAL, "wavlm_posconv: negative size or stride");
  if (K % 2) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_posconv: the kernel size must be even (the reference drops the last frame of an even kernel)");
  if (C % groups || (C / groups) % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_posconv: C / groups must be a multiple of 16");
  if (T > 0 && xp_bs < (int64_t)(T + K - 1) * C) return tdvc_fail(TDVC_EINVAL, "wavlm_posconv: the padded row holds T + K - 1 tokens");
  tdvc_wavlm_gemm_args a = {};
  a.B = B; a.T = T; a.N = C / groups; a.K = K * (C / groups); a.groups = groups; a.seg_len = C / groups; a.epilogue = 1;
  a.x = xp; a.x_bs = xp_bs; a.x_ts = C; a.x_ss = C; a.x_gs = C / groups; a.w = w; a.bias = bias;
  a.res = xp ? xp + (int64_t)(K / 2) * C : nullptr; a.r_bs = xp_bs; a.r_ts = C; a.y = y; a.y_bs = y_bs; a.y_ts = y_ts;
  const char* why;
  const int rc = gemm_check(&a, &why);
  if (rc != TDVC_OK) return tdvc_fail(rc, why);
  if (B == 0 || T == 0) return TDVC_OK;
  if (!bias) return tdvc_fail(TDVC_EINVAL, "wavlm_posconv: null pointer");
  gemm_launch(&a, (hipStream_t)stream);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_wavlm_attention(const float* q, const float* k, const float* v, int64_t bs, int64_t ts, int32_t B, int32_t T, int32_t H, int32_t d,
                                    const float* gate, const float* bias_rel, float* out, int64_t o_bs, int64_t o_ts, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || H < 1 || d < 1 || bs < 0 || ts < 0 || o_bs < 0 || o_ts < 0) return tdvc_fail(TDVC_EINVAL, "wavlm_attention: negative size or stride");
  if (d != 16 && d != 32 && d != 64) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_attention: the head width must be 16, 32 or 64");
  if (T > AT_MAXT) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_attention: more than 4096 tokens");
  if (B > 65535 || H > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "wavlm_attention: B or H > 65535");
  if ((bs | ts | o_bs | o_ts) & 3) return tdvc_fail(TDVC_EINVAL, "wavlm_attention: strides must be multiples of 4 floats");
  if (ts < (int64_t)H * d || o_ts < (int64_t)H * d) return tdvc_fail(TDVC_EINVAL, "wavlm_attention: token stride below H d");
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return tdvc_fail(TDVC_EINVAL, "wavlm_attention: q, k, v and out must be 16-byte aligned");
  if (B == 0 || T == 0) return TDVC_OK;
  if (!q || !k || !v || !gate || !bias_rel || !out) return tdvc_fail(TDVC_EINVAL, "wavlm_attention: null pointer");
  AttnP p;
  p.q = q; p.k = k; p.v = v; p.bs = bs; p.ts = ts; p.T = T; p.H = H; p.gate = gate; p.bias_rel = bias_rel; p.out = out; p.o_bs = o_bs; p.o_ts = o_ts;
  attn_tile_launch<true>(p, B, d, (hipStream_t)stream);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
