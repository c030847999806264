// The backward pass of the CREPE pitch tracker with respect to its input signal (the activation-MSE lambda_f0 term of the reference's
// train.py:439-470), restated in include/tdvc.h. The network is fixed: no weight gradients, and no saved activations either. What
// the backward needs of the forward is the pooling decision of every output (tdvc_crepe_conv_train in pitch_crepe.hip) and the final
// activations.
//
// tdvc_crepe_act_mse     mean((act - target)^2): block partials in float64 over fixed slabs, summed in order by one block. No atomics,
//                        so a graph replay logs the bits of the eager run
// tdvc_crepe_head_bwd    dlogit from the loss (or from a given d act) and the sigmoid, then dx6 = dlogit W: a block per 8 frames x 256
//                        features, the 8 x 360 dlogit in LDS as float64, a thread per feature, float64 sums over the outputs in order
// tdvc_crepe_conv_bwd    one launch per layer: unpool, ReLU mask, BatchNorm scale and the input gradient of the conv, below
// tdvc_crepe_frames_bwd  two launches: a block per frame recomputes mean and deviation and reduces mean(g) and sum(g y) in float64
//                        (pairwise combine of the four waves, as the forward); then a thread per signal sample gathers the frames
//                        that cover it (1024 / hop of them) in float64, in frame order, one rounding. No atomics
// tdvc_roll_bins         util.roll_batches(act, shift, 1) on [B][C][F]
//
// The conv backward is the forward's implicit GEMM on v_mfma_f32_16x16x4_f32 with the roles of the channels exchanged: M = 16 INPUT
// channels, the columns are (frame, input position), the reduction runs over (output channel, tap). dz is never stored: the B operand is
// expanded from dy, the code and the scale while it is staged into LDS (dz[p] = dy[p >> 1] scale if the code names p, else 0: a select,
// so a NaN in an unselected dy never reaches a product). The weights come from a transposed, tap-flipped packing made once per model
// (crepe.py), which turns the correlation into the forward's loop:
//   K = 64, stride 1:  dx[ci][s] = sum_co sum_k' wt[ci][co][k'] dzp[co][s + k'], wt[ci][co][k'] = w[co][ci][63 - k'], dzp the frame behind
//                      32 zeros and in front of 32. Chunk = 2 output channels x 64 taps, xs[channel][frame][LC + 64], the four k of one
//                      MFMA four consecutive taps: the forward's bank pattern (17 consecutive words per 32-lane half)
//   K = 512, stride 4: dx[s] = sum_co sum_p w[co][s + 254 - 4 p] dz[co][p]. With one input channel, M = channel would leave 15 of 16
//                      rows empty; instead the rows are r = s mod 16 and the columns m = s div 16 (64 per frame, 4 frames per block).
//                      With p = 4 m + u the weight A[r][(co, u)] = w[co][r + 254 - 4 u] does not depend on m; u runs over [-64, 68),
//                      padded to CR_L1_U = 136 with zero weights. B[(co, u)][m] = dz[co][4 m + u] is staged as four phase planes
//                      per frame, plane q word w = dz[4 w + q - 64], so that column m and product 4 kk + q meet at plane q, word m + kk:
//                      consecutive words; planes are 112 = 16 mod 32 words apart. Chunk = 1 output channel x 136 products. The
//                      accumulator's four rows of a lane are four consecutive samples: one 16-byte store
// Each chunk is summed from zero and added to the running sum, as in the forward. Fixed order, no atomics: bit-identical from call to
// call, and a frame's gradient does not depend on its batch.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "pitch_crepe.h"
#include "reduce.h"

namespace tdvc {

// ---------------------------------------------------------------------------------------------------------------- loss value
constexpr int CR_MSE_BLOCKS = 256;

struct CrTgt { const float* p; long bs, cs, fs; };                           // target[b][o][f] at p[b bs + o cs + f fs]

__global__ __launch_bounds__(256) void crepe_mse_partial_kernel(const float* act, CrTgt tg, long n, int O, int F, long per, double* part) {
  __shared__ double red[4];
  const long lo = blockIdx.x * per, hi = min(lo + per, n);
  double s = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    const long b = i / ((long)O * F), r = i - b * (long)O * F;
    const long o = r / F, f = r - o * F;
    const double d = (double)act[i] - (double)tg.p[b * tg.bs + o * tg.cs + f * tg.fs];
    s = fma(d, d, s);
  }
  s = block_sum_pairwise(s, red, threadIdx.x);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void crepe_mse_final_kernel(const double* part, int nb, double inv_n, float* out) {
  if (threadIdx.x) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += part[i];
  out[0] = (float)(s * inv_n);
}

// ---------------------------------------------------------------------------------------------------------------- head
constexpr int CR_HF = 8;                                                     // frames per block, as the forward head

// dact == nullptr: dlogit = gL 2 (act - target) / n act (1 - act); else dlogit = dact act (1 - act) (dact dense, the layout of act)
__global__ __launch_bounds__(256) void crepe_head_bwd_kernel(const float* act, CrTgt tg, const float* gL, const float* dact, const float* w, int N,
                                                             int C, int P, int O, int F, double inv_n, float* dx) {
  extern __shared__ double dl[];                                             // [CR_HF][O]
  const int t = threadIdx.x, n0 = blockIdx.x * CR_HF, PC = P * C;
  const double g = dact ? 0.0 : 2.0 * (double)gL[0] * inv_n;
  for (int e = t; e < CR_HF * O; e += 256) {
    const int fr = e / O, o = e - fr * O, n = n0 + fr;
    double v = 0.0;
    if (n < N) {
      const long b = n / F, f = n - b * F;
      const long at = (b * O + o) * F + f;
      const double a = (double)act[at];
      const double up = dact ? (double)dact[at] : g * (a - (double)tg.p[b * tg.bs + o * tg.cs + f * tg.fs]);
      v = up * a * (1.0 - a);
    }
    dl[e] = v;
  }
  __syncthreads();
  const int i = blockIdx.y * 256 + t;                                        // feature l C + c
  if (i >= PC) return;
  double acc[CR_HF];
#pragma unroll
  for (int fr = 0; fr < CR_HF; ++fr) acc[fr] = 0.0;
  for (int o = 0; o < O; ++o) {
    const double wi = (double)w[(long)o * PC + i];
#pragma unroll
    for (int fr = 0; fr < CR_HF; ++fr) acc[fr] = fma(dl[fr * O + o], wi, acc[fr]);
  }
  const int l = i / C, c = i - l * C;
#pragma unroll
  for (int fr = 0; fr < CR_HF; ++fr)
    if (n0 + fr < N) dx[(long)(n0 + fr) * PC + c * P + l] = (float)acc[fr];
}

// ---------------------------------------------------------------------------------------------------------------- conv
struct CrBwdP {
  int N, Cin, Cout;
  const float* dy; const unsigned char* code; const float* scale; const float* wt;
  float* dx;
};

// S = 4: layer 1, LC = 256 conv positions, dx [N][1024]. S = 1: K = 64, dx [N][Cin][LC].
template <int S, int LC>
__global__ __launch_bounds__(CR_THREADS, 2) void crepe_conv_bwd_kernel(CrBwdP p) {
  constexpr int FPB = S == 4 ? 4 : 256 / LC;                     // frames per block
  constexpr int CH = S == 4 ? 1 : 2;                             // output channels per chunk
  constexpr int KCH = S == 4 ? CR_L1_U : CR_KCH;                 // products per chunk and chain
  constexpr int WP = S == 4 ? CR_L1_WP : CR_WP;
  constexpr int LOUT = LC / 2;
  constexpr int LP = LC + 64;                                    // S = 1: words per (channel, frame)
  constexpr int PL = 112, PLU = 64 + CR_L1_U / 4;                // S = 4: plane pitch and the words of a plane that are read (98)
  constexpr int XC = S == 4 ? FPB * 4 * PL : FPB * LP;           // words per chunk channel
  constexpr int XTOT = CH * XC;
  constexpr int XS = XTOT / CR_THREADS;
  constexpr int NWT = 16 * KCH / 4;                              // float4 of weights per chunk
  constexpr int NW = (NWT + CR_THREADS - 1) / CR_THREADS;
  static_assert(S == 4 ? LC == 256 : (LC >= 8 && LC <= 128 && 256 % LC == 0), "geometry");
  static_assert(XTOT % CR_THREADS == 0 && PLU <= PL, "staging shape");
  __shared__ float xs[XTOT];
  __shared__ float ws[16 * WP];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, j = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * FPB, ci0 = blockIdx.y * 16;
  const int R = p.Cout * (S == 4 ? CR_L1_U : 64);                // the reduction's length, a multiple of KCH
  // what this thread stages per chunk: XS words of xs. src: the pooled output that position p of the word belongs to, for output
  // channel 0 of the chunk's first (+ ch CH LOUT per chunk); want: the code that names p
  int src[XS];
  unsigned char want[XS];
#pragma unroll
  for (int sl = 0; sl < XS; ++sl) {
    const int e = t + CR_THREADS * sl;
    int n, cl, pos;
    if constexpr (S == 4) {
      const int fl = e / (4 * PL), r = e - fl * 4 * PL, pl = r / PL, w = r - pl * PL;
      n = n0 + fl; cl = 0; pos = w < PLU ? 4 * w + pl - 64 : -1;
    } else {
      cl = e / XC;
      const int r = e - cl * XC, fl = r / LP;
      n = n0 + fl; pos = r - fl * LP - 32;
    }
    const bool in = pos >= 0 && pos < LC && n < p.N;
    src[sl] = in ? (n * p.Cout + cl) * LOUT + (pos >> 1) : -1;              // N Cout LOUT < 2^31 (checked on the host)
    want[sl] = (pos & 1) ? CR_CODE_ODD : CR_CODE_EVEN;
  }
  const float* wsrc[NW];
#pragma unroll
  for (int sl = 0; sl < NW; ++sl) {
    const int u = min(t + CR_THREADS * sl, NWT - 1), r = u / (KCH / 4);
    wsrc[sl] = p.wt + (long)(ci0 + r) * R + 4 * (u - r * (KCH / 4));
  }
  float xreg[XS];
  float4 wreg[NW];
  auto load = [&](int ch) {                                                 // chunk ch: output channels [CH ch, CH ch + CH)
#pragma unroll
    for (int sl = 0; sl < XS; ++sl) {
      float v = 0.f;
      if (src[sl] >= 0) {
        const int cl = S == 4 ? 0 : (t + CR_THREADS * sl) / XC;
        const int at = src[sl] + ch * CH * LOUT;
        const float g = p.dy[at] * p.scale[ch * CH + cl];
        v = p.code[at] == want[sl] ? g : 0.f;
      }
      xreg[sl] = v;
    }
#pragma unroll
    for (int sl = 0; sl < NW; ++sl) wreg[sl] = *reinterpret_cast<const float4*>(wsrc[sl] + ch * KCH);
  };
  // the column of this lane in accumulator tile nt, as a word offset into one chunk channel of xs
  int coloff[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = 64 * wv + 16 * nt + j;
    coloff[nt] = S == 4 ? wv * 4 * PL + q * PL + 16 * nt + j : (col / LC) * LP + (col % LC) + q;
  }
  cr_f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = cr_f32x4{0.f, 0.f, 0.f, 0.f};
  const int nch = R / KCH;
  load(0);
  for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
    for (int sl = 0; sl < XS; ++sl) xs[t + CR_THREADS * sl] = xreg[sl];
#pragma unroll
    for (int sl = 0; sl < NW; ++sl) {
      const int u = t + CR_THREADS * sl, r = u / (KCH / 4);
      if (NWT % CR_THREADS == 0 || u < NWT) {
        float* d = ws + r * WP + 4 * (u - r * (KCH / 4));
        d[0] = wreg[sl].x; d[1] = wreg[sl].y; d[2] = wreg[sl].z; d[3] = wreg[sl].w;
      }
    }
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1);
    cr_f32x4 part[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) part[nt] = cr_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KCH / 4; ++kk) {
      const float a = ws[j * WP + 4 * kk + q];
      // S = 4: plane q, word m + kk. S = 1: product 4 kk + q is channel kk / 16 of the chunk, flipped tap 4 (kk % 16) + q
      const int step = S == 4 ? kk : (kk / 16) * XC + 4 * (kk % 16);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xs[coloff[nt] + step], part[nt], 0, 0, 0);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] += part[nt];
    __syncthreads();
  }
  if constexpr (S == 4) {                                                   // rows 4 q .. 4 q + 3 of column m: samples 16 m + 4 q ..
    const int n = n0 + wv;
    if (n < p.N) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        *reinterpret_cast<float4*>(p.dx + (long)n * CR_WIN + 16 * (16 * nt + j) + 4 * q) = make_float4(acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
    }
  } else {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int col = 64 * wv + 16 * nt + j, n = n0 + col / LC, pos = col % LC;
      if (n < p.N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p.dx[((long)n * p.Cin + ci0 + 4 * q + r) * LC + pos] = acc[nt][r];
      }
    }
  }
}

template <int S, int LC>
static void crepe_conv_bwd_launch(const CrBwdP& p, hipStream_t st) {
  constexpr int FPB = S == 4 ? 4 : 256 / LC;
  hipLaunchKernelGGL((crepe_conv_bwd_kernel<S, LC>), dim3((p.N + FPB - 1) / FPB, S == 4 ? 1 : p.Cin / 16), dim3(CR_THREADS), 0, st, p);
}

// ---------------------------------------------------------------------------------------------------------------- frames
// stats[n] = (mean, den, mean(g), sum(g y) / 1023 or 0 where the deviation is at or below 1e-10)
__global__ __launch_bounds__(256) void crepe_frames_bwd_stats_kernel(const float* x, long x_bs, int T, int hop, int F, const float* g, double* stats) {
  __shared__ double red[4];
  const int t = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  const float* row = x + b * x_bs;
  const long fn = (long)b * F + f, q0 = (long)f * hop - CR_WIN / 2;
  const float* gr = g + fn * CR_WIN;
  double v[4], gv[4], s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long q = q0 + t + 256 * k;
    v[k] = q >= 0 && q < T ? (double)row[q] : 0.0;
    s += v[k];
  }
  const double mean = block_sum_pairwise(s, red, t) / (double)CR_WIN;       // the forward's two passes, in its order
  __syncthreads();
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[k] -= mean; ss = fma(v[k], v[k], ss); }
  const double sd = sqrt(block_sum_pairwise(ss, red, t) / (double)(CR_WIN - 1));
  const double den = fmax(1e-10, sd);
  __syncthreads();
  double sg = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { gv[k] = (double)gr[t + 256 * k]; sg += gv[k]; }
  const double mg = block_sum_pairwise(sg, red, t) / (double)CR_WIN;
  __syncthreads();
  double sgy = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) sgy = fma(gv[k], v[k] / den, sgy);
  const double c = block_sum_pairwise(sgy, red, t) / (double)(CR_WIN - 1);
  if (t == 0) {
    double* o = stats + 4 * fn;
    o[0] = mean; o[1] = den; o[2] = mg; o[3] = sd > 1e-10 ? c : 0.0;
  }
}

__global__ __launch_bounds__(256) void crepe_frames_bwd_gather_kernel(const float* x, long x_bs, int T, int hop, int F, const float* g,
                                                                     const double* stats, float* dx, long dx_bs) {
  const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (q >= T) return;
  const long pos = (long)q + CR_WIN / 2;                                    // index in the padded row
  const long lo = pos < CR_WIN ? 0 : (pos - CR_WIN) / hop + 1;              // first and last frame whose window holds pos
  const long hi = min(pos / hop, (long)F - 1);
  const double xv = (double)x[b * x_bs + q];
  double s = 0.0;
  for (long f = lo; f <= hi; ++f) {
    const long fn = (long)b * F + f;
    const double* st = stats + 4 * fn;
    const double y = (xv - st[0]) / st[1];
    s += ((double)g[fn * CR_WIN + (pos - f * hop)] - st[2] - y * st[3]) / st[1];
  }
  dx[b * dx_bs + q] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------- roll
__global__ __launch_bounds__(256) void crepe_roll_bins_kernel(const float* x, long x_bs, long x_cs, const int64_t* shift, float* y, int C, int F) {
  const int b = blockIdx.y;
  long sft = shift[b] % C;
  if (sft < 0) sft += C;
  const long n = (long)C * F;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long k = i / F, f = i - k * F;
    long srck = k - sft;
    if (srck < 0) srck += C;
    y[b * n + i] = x[b * x_bs + srck * x_cs + f];
  }
}

static int crepe_tgt_check(const char* who, int32_t B, int32_t O, int32_t F) {
  if (B < 0 || O < 1 || F < 1) return tdvc_fail(TDVC_EINVAL, who);
  if (B > 65535 || O > (1 << 16) || (double)B * O * F > 2147483647.0) return tdvc_fail(TDVC_EUNSUPPORTED, who);
  return TDVC_OK;
}

}  // namespace tdvc

extern "C" size_t tdvc_crepe_act_mse_workspace(void) { return tdvc::CR_MSE_BLOCKS * sizeof(double); }

extern "C" int tdvc_crepe_act_mse(const float* act, const float* target, int64_t t_bs, int64_t t_cs, int64_t t_fs, int32_t B, int32_t O, int32_t F,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (int rc = crepe_tgt_check("crepe_act_mse: B, O or F negative, zero or beyond 65535 rows, 2^16 outputs, 2^31 elements", B, O, F)) return rc;
  if (t_bs < 0 || t_cs < 0 || t_fs < 0) return tdvc_fail(TDVC_EINVAL, "crepe_act_mse: negative stride");
  if (B == 0) return tdvc_fail(TDVC_EINVAL, "crepe_act_mse: the mean over no element");
  if (!act || !target || !out) return tdvc_fail(TDVC_EINVAL, "crepe_act_mse: null pointer");
  if (!workspace || workspace_bytes < tdvc_crepe_act_mse_workspace()) return tdvc_fail(TDVC_EWORKSPACE, "crepe_act_mse: workspace missing or too small");
  const long n = (long)B * O * F;
  const long per = ((n + CR_MSE_BLOCKS - 1) / CR_MSE_BLOCKS + 255) / 256 * 256;      // a slab per block, whole rounds of the block
  const int nb = (int)((n + per - 1) / per);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(crepe_mse_partial_kernel, dim3(nb), dim3(256), 0, st, act, CrTgt{target, (long)t_bs, (long)t_cs, (long)t_fs}, n, O, F, per,
                     static_cast<double*>(workspace));
  TDVC_CHECK_LAUNCH();
  hipLaunchKernelGGL(crepe_mse_final_kernel, dim3(1), dim3(64), 0, st, static_cast<const double*>(workspace), nb, 1.0 / (double)n, out);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_crepe_head_bwd(const float* act, const float* target, int64_t t_bs, int64_t t_cs, int64_t t_fs, const float* gL,
                                   const float* dact, const float* w, int32_t N, int32_t C, int32_t P, int32_t O, int32_t F, float* dx,
                                   void* stream) {
  using namespace tdvc;
  if (N < 0 || C < 1 || P < 1 || O < 1 || F < 1) return tdvc_fail(TDVC_EINVAL, "crepe_head_bwd: negative N, or C, P, O or F below 1");
  if (t_bs < 0 || t_cs < 0 || t_fs < 0) return tdvc_fail(TDVC_EINVAL, "crepe_head_bwd: negative stride");
  if (C % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_head_bwd: C must be a multiple of 16");
  if (N % F) return tdvc_fail(TDVC_EINVAL, "crepe_head_bwd: N must be a multiple of the frames per row F");
  if (O > 512 || N > (1 << 22) || (double)N * C * P > 2147483647.0 || (double)N * O > 2147483647.0 || (double)C * P > (1 << 24))
    return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_head_bwd: more than 512 outputs, 2^22 frames, 2^24 features or 2^31 elements");
  if (N == 0) return TDVC_OK;
  if (!act || !w || !dx || (dact ? (target || gL) : (!target || !gL)))
    return tdvc_fail(TDVC_EINVAL, "crepe_head_bwd: null pointer (the loss form takes target and gL, the plain form d act alone)");
  const int PC = P * C;
  hipLaunchKernelGGL(crepe_head_bwd_kernel, dim3((N + CR_HF - 1) / CR_HF, (PC + 255) / 256), dim3(256), CR_HF * O * sizeof(double), (hipStream_t)stream,
                     act, CrTgt{target, (long)t_bs, (long)t_cs, (long)t_fs}, gL, dact, w, N, C, P, O, F, 1.0 / ((double)N * O), dx);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_crepe_conv_bwd(const tdvc_crepe_conv_bwd_args* a, void* stream) {
  using namespace tdvc;
  if (!a) return tdvc_fail(TDVC_EINVAL, "crepe_conv_bwd: null arguments");
  if (a->N < 0 || a->Cin < 1 || a->Cout < 1) return tdvc_fail(TDVC_EINVAL, "crepe_conv_bwd: negative N or a channel count below 1");
  const bool first = a->stride == 4 && a->K == 512 && a->Cin == 1 && a->Lin == CR_WIN;
  const bool later = a->stride == 1 && a->K == 64 && (a->Lin == 128 || a->Lin == 64 || a->Lin == 32 || a->Lin == 16 || a->Lin == 8);
  if (!first && !later)
    return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_conv_bwd: the geometry must be Cin 1, K 512, stride 4 on 1024 samples, or K 64, stride 1 on 128, 64, 32, 16 or 8 positions");
  if (a->Cout % 16 || (later && a->Cin % 16)) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_conv_bwd: channel counts must be multiples of 16");
  const int lc = first ? 256 : a->Lin;
  if (a->Cout > (1 << 16) || a->Cin > (1 << 16) || (double)a->N * a->Cin * a->Lin > 2147483647.0 || (double)a->N * a->Cout * (lc / 2) > 2147483647.0 ||
      a->N > (1 << 22))
    return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_conv_bwd: more than 2^16 channels, 2^22 frames or 2^31 elements");
  if (a->N == 0) return TDVC_OK;
  if (!a->dy || !a->code || !a->scale || !a->wt || !a->dx) return tdvc_fail(TDVC_EINVAL, "crepe_conv_bwd: null pointer");
  if (((uintptr_t)a->wt & 15) != 0 || ((uintptr_t)a->dx & 15) != 0) return tdvc_fail(TDVC_EINVAL, "crepe_conv_bwd: wt and dx must be 16-byte aligned");
  CrBwdP p;
  p.N = a->N; p.Cin = a->Cin; p.Cout = a->Cout; p.dy = a->dy; p.code = a->code; p.scale = a->scale; p.wt = a->wt; p.dx = a->dx;
  hipStream_t st = (hipStream_t)stream;
  if (first) crepe_conv_bwd_launch<4, 256>(p, st);
  else if (lc == 128) crepe_conv_bwd_launch<1, 128>(p, st);
  else if (lc == 64) crepe_conv_bwd_launch<1, 64>(p, st);
  else if (lc == 32) crepe_conv_bwd_launch<1, 32>(p, st);
  else if (lc == 16) crepe_conv_bwd_launch<1, 16>(p, st);
  else crepe_conv_bwd_launch<1, 8>(p, st);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" size_t tdvc_crepe_frames_bwd_workspace(int32_t B, int32_t F) {
  if (B < 1 || F < 1) return 0;
  return (size_t)B * (size_t)F * 4 * sizeof(double);
}

extern "C" int tdvc_crepe_frames_bwd(const float* signal, int64_t s_bs, int32_t T, int32_t B, int32_t hop, int32_t F, const float* g, float* dsignal,
                                     int64_t d_bs, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || s_bs < 0 || d_bs < 0) return tdvc_fail(TDVC_EINVAL, "crepe_frames_bwd: negative B, T or stride");
  if (hop < 1) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames_bwd: hop must be at least 1");
  if (T < 1) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames_bwd: rows with no sample");
  if (B > 65535 || T > (1 << 28)) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames_bwd: B > 65535 or T > 2^28");
  if (F != 1 + T / hop) return tdvc_fail(TDVC_EINVAL, "crepe_frames_bwd: F must be 1 + T / hop");
  if ((double)B * F * CR_WIN > 2147483647.0 * 4) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames_bwd: more than 2^33 frame elements");
  if (B == 0) return TDVC_OK;
  if (!signal || !g || !dsignal) return tdvc_fail(TDVC_EINVAL, "crepe_frames_bwd: null pointer");
  if (!workspace || workspace_bytes < tdvc_crepe_frames_bwd_workspace(B, F)) return tdvc_fail(TDVC_EWORKSPACE, "crepe_frames_bwd: workspace missing or too small");
  hipStream_t st = (hipStream_t)stream;
  double* stats = static_cast<double*>(workspace);
  hipLaunchKernelGGL(crepe_frames_bwd_stats_kernel, dim3(F, B), dim3(256), 0, st, signal, (long)s_bs, T, hop, F, g, stats);
  TDVC_CHECK_LAUNCH();
  hipLaunchKernelGGL(crepe_frames_bwd_gather_kernel, dim3((T + 255) / 256, B), dim3(256), 0, st, signal, (long)s_bs, T, hop, F, g, stats, dsignal, (long)d_bs);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_roll_bins(const float* x, int64_t x_bs, int64_t x_cs, const int64_t* shift, float* y, int32_t B, int32_t C, int32_t F, void* stream) {
  using namespace tdvc;
  if (B < 0 || C < 1 || F < 1 || x_bs < 0 || x_cs < 0) return tdvc_fail(TDVC_EINVAL, "roll_bins: negative B or stride, or C or F below 1");
  if (B > 65535 || (double)B * C * F > 2147483647.0) return tdvc_fail(TDVC_EUNSUPPORTED, "roll_bins: B > 65535 or more than 2^31 elements");
  if (B == 0) return TDVC_OK;
  if (!x || !shift || !y) return tdvc_fail(TDVC_EINVAL, "roll_bins: null pointer");
  hipLaunchKernelGGL(crepe_roll_bins_kernel, dim3(tdvc_grid((long)C * F, 256, 256), B), dim3(256), 0, (hipStream_t)stream, x, (long)x_bs, (long)x_cs, shift, y, C, F);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
