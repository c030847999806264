// Backward of the soft YIN pitch tracker (pitch_yin.hip with soft != 0): upstream gy [B][n_frames] -> dx [B][T], two launches.
//
// (a) yin_soft_bwd_frame_kernel, one 256-thread block per (sample, frame). A frame with gy == 0 writes zeros at once. Otherwise
//     the block recomputes d, S, c and the softmax with the forward's own device code (pitch_yin.h: same bits, so the same
//     on/off decision and the same f0), and a frame that is off (or has f0 == 0) writes zeros too. A live frame continues with
//       g_tau = gy * (-f0^2 / sr)
//       gc_m  = g_tau * (-100) * alpha_k * (k - tau)                      k = m - 1 - tau_min >= 0, else 0
//       G_m   = gc_m * m / den_m - sum_{j >= m, S_j > floor} gc_j * c_j / S_j          (c_j = j d_j / S_j)
//       du_n  = 2 * sum_m G_m * [ (u_n - u_{n+m}) 1(n+m < L) + (u_n - u_{n-m}) 1(n-m >= 0) ]
//     G: every thread owns the four lags it owned in the CMDF, the suffix sum is a wave64 shuffle scan plus one cross-wave step.
//     du: a direct correlation of G with the LDS-resident frame. A work item is four consecutive n and a slice of m; it walks m
//     four at a time with two sliding register windows, u[n0+m ..] moving up and u[n0-m ..] moving down, so one step is three
//     ds_read_b128 (G_m..m+3: the same address in every lane of a slice = broadcast; one new float4 per window) for 16 (n, m)
//     pairs. The differences are taken BEFORE the multiply; u_n * sum G - sum G u would cancel. Every n has one side that is
//     complete and one that is cut off by the frame edge, so a step runs in one of four forms, chosen per wave (no divergence):
//     both sides whole, only the upper / only the lower side alive, or both masked (the steps around the diagonals). Sums run in
//     blocks of 16 lags folded with a compensated add, like the forward's; the m slices are folded in order through LDS.
//     The block writes du[b][f][0 .. L) to the workspace.
// (b) yin_soft_bwd_gather_kernel: dx[b][t] = sum over the frames f whose window covers t of du[b][f][t + L/2 - f*stride], in
//     ascending f. Every element of dx is written; the zero extension and both pads of the forward receive nothing.
// No atomics: every sum has a fixed order and two runs give identical bits.
//
// Built with -fno-slp-vectorize like pitch_yin.o (csrc/Makefile): the correlation loop is the same scalar sub + fma pattern, 53 VGPRs
// scalar against 96 packed.
#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include "pitch_yin.h"

namespace tdvc {

constexpr int YIN_G_FLOATS = YIN_TAU_CAP + 8;       // G[0 .. roundup4(tau_max)) and a zero tail
constexpr int YIN_PART_FLOATS = 4096;               // m slices x roundup4(L) partial du; also holds dpart and the CMDF before that
constexpr int YIN_BWD_MAX_SLICES = 8;
static_assert(YIN_PART_FLOATS >= YIN_D_FLOATS + YIN_TAU_CAP, "dpart and the CMDF share the partial-sum buffer");
static_assert(YIN_PART_FLOATS >= 2 * YIN_TAU_CAP, "one slice of a full-length frame must fit");

struct YinBwdP {
  const float* x; long x_bs;
  int T, tau_min, tau_max, stride, n_frames;
  int NG, NC;                                       // the forward's split of the difference function
  int NGn, NCm, mslice;                             // correlation: groups of 4 n; slices of m; lags per slice (multiple of 4)
  float threshold, sample_rate;
  const float* gy; float* du;
};

// One step of the correlation: lags m0 .. m0+3 against n0 .. n0+3.  F = u[n0+m0 .. n0+m0+8), Bw = u[n0-m0-4 .. n0-m0+4).
// FW / BW: the side takes part; MASK: each term is checked against the frame edge (tf = L - n0 - m0, tb = n0 - m0).
template <bool FW, bool BW, bool MASK>
__device__ __forceinline__ void yin_bwd_step(float (&blk)[4], const float (&a)[4], const float (&G)[4], const float (&F)[8],
                                             const float (&Bw)[8], int tf, int tb) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = 0.f;
      if (FW) {
        float df = a[i] - F[i + r];                            // u[n0+i] - u[n0+i+m0+r]
        if (MASK) df = (i + r < tf) ? df : 0.f;
        s = df;
      }
      if (BW) {
        float db = a[i] - Bw[4 + i - r];                       // u[n0+i] - u[n0+i-m0-r]
        if (MASK) db = (r - i <= tb) ? db : 0.f;
        s = FW ? s + db : db;
      }
      blk[i] = fmaf(G[r], s, blk[i]);
    }
  }
}

__global__ __launch_bounds__(YIN_THREADS) void yin_soft_bwd_frame_kernel(YinBwdP p) {
  __shared__ __attribute__((aligned(16))) float u[YIN_U_FLOATS];
  __shared__ __attribute__((aligned(16))) float Gl[YIN_G_FLOATS];
  __shared__ __attribute__((aligned(16))) float part[YIN_PART_FLOATS];
  __shared__ float redf[YIN_RED_SLOTS * YIN_WAVES];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.n_frames, f = blockIdx.x - b * p.n_frames;
  const int L = 2 * p.tau_max;
  const long fr = (long)b * p.n_frames + f;
  float* du = p.du + fr * L;
  const float gy = p.gy[fr];
  if (gy == 0.f) {                                              // block-uniform
    for (int j = tid; j < L; j += YIN_THREADS) du[j] = 0.f;
    return;
  }

  // ---- the forward's phases, on the forward's code; the frame stays in u, the CMDF goes behind dpart
  float* dpart = part;
  float* cl = part + YIN_D_FLOATS;
  yin_stage_frame(p.x, p.x_bs, p.T, p.tau_max, p.stride, b, f, u);
  __syncthreads();
  yin_difference(u, dpart, L, p.NG, p.NC);
  __syncthreads();
  const int n1 = p.tau_max - 1;
  const int n = n1 - p.tau_min;
  float d[4], S[4];
  yin_cmdf(dpart, redf, cl, p.tau_min, p.tau_max, p.NG, p.NC, d, S);
  __syncthreads();
  float mn, se, sk;
  yin_soft_search(cl, n, redf, mn, se, sk);
  const float tau = (mn < p.threshold) ? sk / se : 0.f;
  const float f0 = yin_f0_of_tau(tau, p.tau_min, p.sample_rate);
  if (!(f0 > 0.f)) {                                            // off, or tau == 0: block-uniform (every lane holds the same sums)
    for (int j = tid; j < L; j += YIN_THREADS) du[j] = 0.f;
    return;
  }

  // ---- G[m], m = k + 1, k = 4*tid .. 4*tid+3
  {
    const float coef = gy * (-(f0 * f0) / p.sample_rate) * -100.f / se;
    float first[4], suf[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * tid + e, kk = k - p.tau_min;
      float gc = 0.f, c = 0.f;
      if (kk >= 0 && k < n1) {
        c = cl[kk];
        gc = coef * yin_soft_weight(c, mn) * ((float)kk - tau);
      }
      first[e] = gc * (float)(k + 1) / fmaxf(S[e], YIN_FLOOR);
      suf[e] = (S[e] > YIN_FLOOR) ? gc * c / S[e] : 0.f;       // gc_j j d_j / S_j^2 = gc_j c_j / S_j; no term where the floor is active
    }
    suf[2] += suf[3]; suf[1] += suf[2]; suf[0] += suf[1];       // suffix sums inside the thread
    const float tot = suf[0];
    float incl = tot;                                           // wave64 inclusive suffix scan of the thread totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      float t = __shfl_down(incl, o, 64);
      if ((tid & 63) + o < 64) incl += t;
    }
    if ((tid & 63) == 0) redf[4 * YIN_WAVES + (tid >> 6)] = incl;
    __syncthreads();
    float after = 0.f;
    for (int w = YIN_WAVES - 1; w > (tid >> 6); --w) after += redf[4 * YIN_WAVES + w];
    after += incl - tot;                                        // everything behind this thread's four values
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * tid + e;                                // Gl[1 .. 1024]
      Gl[k + 1] = (k < n1) ? first[e] - (after + suf[e]) : 0.f;
    }
    if (tid == 0) Gl[0] = 0.f;
    if (tid < YIN_G_FLOATS - (YIN_R * YIN_THREADS + 1)) Gl[YIN_R * YIN_THREADS + 1 + tid] = 0.f;
  }
  __syncthreads();                                              // G complete; dpart and the CMDF are dead, `part` is free

  // ---- du: work item = (slice c of m, group g of four n)
  const int Lp = (L + 3) & ~3;
  const int M4 = (p.tau_max + 3) & ~3;
  const float4* u4 = reinterpret_cast<const float4*>(u);
  const float4* G4 = reinterpret_cast<const float4*>(Gl);
  constexpr int U4MAX = YIN_U_FLOATS / 4 - 1;
  const int items = p.NGn * p.NCm;
  for (int item = tid; item < items; item += YIN_THREADS) {
    const int g = item % p.NGn, c = item / p.NGn;
    const int n0 = 4 * g;
    const int ma = c * p.mslice, mb = min(ma + p.mslice, M4);
    float a[4], F[8], Bw[8], sum[4], comp[4], blk[4];
    {
      float4 av = u4[g];
      a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] = comp[i] = blk[i] = 0.f;
    // windows at m0 = ma: F[0..4) and Bw[4..8) are held, F[4..8) and Bw[0..4) are read in the step. An index outside the
    // LDS image is clamped: what it reads belongs to terms beyond the frame edge, which only the masked form ever meets.
    {
      float4 w = u4[min((n0 + ma) >> 2, U4MAX)];
      F[0] = w.x; F[1] = w.y; F[2] = w.z; F[3] = w.w;
      w = u4[max((n0 - ma) >> 2, 0)];
      Bw[4] = w.x; Bw[5] = w.y; Bw[6] = w.z; Bw[7] = w.w;
    }
    int cnt = 0;
    for (int m0 = ma; m0 < mb; m0 += 4) {
      float G[4];
      {
        float4 gv = G4[m0 >> 2];
        G[0] = gv.x; G[1] = gv.y; G[2] = gv.z; G[3] = gv.w;
        float4 w = u4[min(((n0 + m0) >> 2) + 1, U4MAX)];
        F[4] = w.x; F[5] = w.y; F[6] = w.z; F[7] = w.w;
        w = u4[max(((n0 - m0) >> 2) - 1, 0)];
        Bw[0] = w.x; Bw[1] = w.y; Bw[2] = w.z; Bw[3] = w.w;
      }
      const int tf = L - n0 - m0, tb = n0 - m0;                 // term (i, r) is inside the frame iff i + r < tf / r - i <= tb
      const bool fw_all = tf >= 7, fw_none = tf <= 0, bw_all = tb >= 3, bw_none = tb <= -4;
      if (__all(fw_all && bw_all)) yin_bwd_step<true, true, false>(blk, a, G, F, Bw, tf, tb);
      else if (__all(fw_all && bw_none)) yin_bwd_step<true, false, false>(blk, a, G, F, Bw, tf, tb);
      else if (__all(fw_none && bw_all)) yin_bwd_step<false, true, false>(blk, a, G, F, Bw, tf, tb);
      else yin_bwd_step<true, true, true>(blk, a, G, F, Bw, tf, tb);
#pragma unroll
      for (int q = 0; q < 4; ++q) { F[q] = F[q + 4]; Bw[q + 4] = Bw[q]; }
      if (++cnt == 4) {                                         // compensated add of a block of 16 lags
        cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float y = blk[i] - comp[i];
          float t = sum[i] + y;
          comp[i] = (t - sum[i]) - y;
          sum[i] = t;
          blk[i] = 0.f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += blk[i] - comp[i];     // the open block
    reinterpret_cast<float4*>(part)[(c * Lp + n0) >> 2] = make_float4(sum[0], sum[1], sum[2], sum[3]);
  }
  __syncthreads();
  for (int j = tid; j < L; j += YIN_THREADS) {
    float s = part[j];
    for (int c = 1; c < p.NCm; ++c) s += part[c * Lp + j];      // slices in order
    du[j] = 2.f * s;
  }
}

__global__ __launch_bounds__(256) void yin_soft_bwd_gather_kernel(const float* __restrict__ du, float* __restrict__ dx, int B, int T,
                                                                  int L, int stride, int n_frames) {
  const long total = (long)B * T;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long b = idx / T;
    const long pos = idx - b * T + L / 2;                       // index in the padded signal
    const long lo = pos - L + 1 <= 0 ? 0 : (pos - L + stride) / stride;      // first and last frame whose window holds pos
    const long hi = min(pos / stride, (long)n_frames - 1);
    const float* row = du + b * n_frames * (long)L;
    float s = 0.f;
    for (long f = lo; f <= hi; ++f) s += row[f * L + (pos - f * stride)];
    dx[idx] = s;
  }
}

static int yin_bwd_check(int32_t B, int32_t T, int32_t tau_min, int32_t tau_max, int32_t stride, int64_t x_bs, float sample_rate) {
  if (T < 1) return tdvc_fail(TDVC_EINVAL, "yin_soft_bwd: T must be >= 1");
  if (stride < 1) return tdvc_fail(TDVC_EINVAL, "yin_soft_bwd: stride must be >= 1");
  if (tau_min < 0 || (long)tau_max - 1 - tau_min < 2) return tdvc_fail(TDVC_EINVAL, "yin_soft_bwd: needs 0 <= tau_min and tau_max - 1 - tau_min >= 2");
  if (tau_max > YIN_TAU_CAP) return tdvc_fail(TDVC_EUNSUPPORTED, "yin_soft_bwd: tau_max above 1024 (the frame no longer fits the kernel's LDS image)");
  if (B < 1 || x_bs < 0 || !(sample_rate > 0.f)) return tdvc_fail(TDVC_EINVAL, "yin_soft_bwd: bad batch, batch stride or sample rate");
  return TDVC_OK;
}

}  // namespace tdvc

extern "C" size_t tdvc_yin_soft_bwd_workspace(int32_t B, int32_t T, int32_t tau_max, int32_t stride) {
  const int nf = tdvc_yin_num_frames(T, tau_max, stride);
  if (B < 1 || nf < 1) return 0;
  return (size_t)B * (size_t)nf * (size_t)(2 * (long)tau_max) * sizeof(float);
}

extern "C" int tdvc_yin_soft_bwd(const float* x, int64_t x_bs, int32_t B, int32_t T, int32_t tau_min, int32_t tau_max, int32_t stride,
                                 float threshold, float sample_rate, const float* gy, float* dx, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  using namespace tdvc;
  if (int rc = yin_bwd_check(B, T, tau_min, tau_max, stride, x_bs, sample_rate)) return rc;
  if (!x || !gy || !dx) return tdvc_fail(TDVC_EINVAL, "yin_soft_bwd: null pointer");
  const int nf = tdvc_yin_num_frames(T, tau_max, stride);
  if ((long)B * nf > INT_MAX) return tdvc_fail(TDVC_EUNSUPPORTED, "yin_soft_bwd: more than 2^31-1 frames in one call");
  if (!workspace) return tdvc_fail(TDVC_EWORKSPACE, "yin_soft_bwd: workspace needed (tdvc_yin_soft_bwd_workspace)");
  if (workspace_bytes < tdvc_yin_soft_bwd_workspace(B, T, tau_max, stride)) return tdvc_fail(TDVC_EWORKSPACE, "yin_soft_bwd: workspace too small");
  const int L = 2 * tau_max, Lp = (L + 3) & ~3, M4 = (tau_max + 3) & ~3;
  YinBwdP p;
  p.x = x; p.x_bs = x_bs; p.T = T; p.tau_min = tau_min; p.tau_max = tau_max; p.stride = stride; p.n_frames = nf;
  p.NG = (tau_max + YIN_R - 1) / YIN_R;
  p.NC = YIN_THREADS / p.NG;
  // m slices: the count (within the LDS the partial sums have) that leaves the fewest threads idle in the last round of items
  p.NGn = Lp / 4;
  const int max_slices = min(min(YIN_BWD_MAX_SLICES, YIN_PART_FLOATS / Lp), M4 / 4);
  int best = 1; long best_num = 0, best_den = 1;                // efficiency = items / (256 * rounds), compared as fractions
  for (int s = 1; s <= max_slices; ++s) {
    const long items = (long)p.NGn * s, rounds = (items + YIN_THREADS - 1) / YIN_THREADS;
    if (items * best_den > best_num * rounds) { best = s; best_num = items; best_den = rounds; }
  }
  p.NCm = best;
  p.mslice = ((M4 / 4 + best - 1) / best) * 4;
  p.threshold = threshold; p.sample_rate = sample_rate;
  p.gy = gy; p.du = static_cast<float*>(workspace);
  auto k = yin_soft_bwd_frame_kernel;
  TDVC_TRACE(k);
  hipLaunchKernelGGL(k, dim3(B * nf), dim3(YIN_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  auto kg = yin_soft_bwd_gather_kernel;
  TDVC_TRACE(kg);
  hipLaunchKernelGGL(kg, dim3(tdvc_grid((long)B * T, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, p.du, dx, B, T, L, stride, nf);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
