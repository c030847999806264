// Speaker recognition with speechbrain's ECAPA-TDNN (the reference's test_scripts/mls-pt/test_speaker_rec.py), restated in
// include/tdvc.h: Fbank(80) with sentence mean normalisation, the ECAPA-TDNN embedding network, all of it length-aware: a row of a
// padded batch is evaluated as if it were alone.
//
// tdvc_fbank       pass 1, one block per 8 frames of a row: Hamming window, a direct 400-point float64 DFT against a cos/sin table
//                  in LDS, power (dft400.h), the mel sums, 10 log10(max(., 1e-10)) into the workspace and the block's maximum; pass 2, one
//                  block per (band, row): the row maximum folded from the block maxima, the M - 80 floor, the mean over the row's
//                  frames in a fixed order, one rounding at the store; writes the row's frame count
// tdvc_tdnn_fwd    the reflect-padded, length-aware Conv1d as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32), below
// tdvc_se_block    mean over the row's frames (a wave per channel), the two matrix-vector products (a wave per output), out = g x +
//                  residual
// tdvc_asp_pool    global-context statistics (a wave per channel), the time-constant part of the 9C -> A product as a per-row
//                  bias, two tdvc_tdnn_fwd launches, then softmax over the row's frames and the weighted statistics (a wave per
//                  channel)
// tdvc_ecapa_head  folded asp_bn + fc, a wave per output
//
// The TDNN kernel. A workgroup of 256 threads (4 waves) owns 64 output channels x 64 frames of one row; wave w owns the channels
// [16 w, 16 w + 16) as four 16 x 16 accumulator tiles over the frames, so that four independent MFMA chains hide the 40-cycle
// dependent latency of the 32-cycle instruction. The reduction runs over chunks of KC input channels (32 for K = 1, 16 for K = 3 and
// 5): the chunk's inputs are gathered into LDS as xs[KC][64 + 2 pad] with the reflect index of the ROW'S OWN frame count n (frames
// at and past n are never read; a second input is added here), its weights as ws[64][KC K + 1]. xs rows are 80 floats apart: lanes
// 0..15 and 16..31 of a ds_read_b32 (one 32-lane group) then fall into disjoint halves of the 32 banks. The next chunk is loaded
// into registers (weights as float4) before the MFMAs of the current one and stored to LDS behind them. Every MFMA of a chunk is
// issued unconditionally (columns past the row's end multiply staged zeros and are not stored): with a branch per frame tile
// around each MFMA the LDS reads could not be scheduled ahead and the MFA layer ran at 28 instead of 79 TFLOP/s
// (profiles/ecapa_bench.txt). Each chunk is summed from zero (KC K products per chain) and then added to the
// running sum, which keeps the rounding of a long reduction (3072 products in the MFA layer) at that of a blocked summation. No
// atomics, one fixed order: bit-identical from call to call, and a row's result does not depend on the batch it is in (a workgroup
// sees one row only).
// The small kernels accumulate in float64 (their cost is nothing beside the GEMMs) and round once.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include "dft400.h"
#include "reduce.h"

namespace tdvc {

constexpr int FB_MAXMEL = 128;
constexpr int TD_TN = 64, TD_TM = 64, TD_XW = 80, TD_THREADS = 256;
constexpr int SE_MAXC = 65532;      // grid.y of the apply launch

typedef float ec_f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------------ Fbank
struct FbankP {
  const float* x; long x_bs;
  const int* lengths; int T, F, M, nblk;
  const double* tab;      // cos[400], sin[400], hamming[400], fb[M][201]
  double* db;             // [B][M][F]
  double* bmax;           // [B][nblk]
  float* out; long o_bs, o_cs;
  int* frames;
};

__global__ __launch_bounds__(256) void fbank_db_kernel(FbankP p) {
  __shared__ double cs[2 * DFT_NFFT];
  __shared__ double xw[DFT_FR][DFT_NFFT];
  __shared__ double pw[DFT_FR][DFT_BINS];
  __shared__ double red[4];
  const int t = threadIdx.x, b = blockIdx.y;
  const int f0 = blockIdx.x * DFT_FR;
  const int n = row_len(p.lengths, b, p.T);
  const int nfr = 1 + n / DFT_HOP;
  if (f0 >= nfr) {                                                          // uniform: nothing of this row is read here
    if (t == 0) p.bmax[(long)b * p.nblk + blockIdx.x] = -INFINITY;
    return;
  }
  const float* row = p.x + b * p.x_bs;
  for (int i = t; i < 2 * DFT_NFFT; i += 256) cs[i] = p.tab[i];
  for (int idx = t; idx < DFT_FR * DFT_NFFT; idx += 256) {
    const int fr = idx / DFT_NFFT, i = idx - fr * DFT_NFFT;
    const long q = (long)(f0 + fr) * DFT_HOP - DFT_NFFT / 2 + i;
    double v = 0.0;
    if (f0 + fr < nfr && q >= 0 && q < n) v = (double)row[q] * p.tab[DFT_TAB_WINDOW + i];
    xw[fr][i] = v;
  }
  __syncthreads();
  dft400_power<256>(cs, xw, pw, t);
  __syncthreads();
  const double* fb = p.tab + DFT_TAB_FB;
  double mx = -INFINITY;
  for (int item = t; item < DFT_FR * p.M; item += 256) {
    const int m = item / DFT_FR, fr = item - m * DFT_FR;
    const int f = f0 + fr;
    if (f >= nfr) continue;
    double acc = 0.0;
    for (int k = 0; k < DFT_BINS; ++k) acc = fma(fb[m * DFT_BINS + k], pw[fr][k], acc);
    const double d = 10.0 * log10(fmax(acc, 1e-10));
    p.db[((long)b * p.M + m) * p.F + f] = d;
    mx = fmax(mx, d);
  }
  mx = block_max<4>(mx, red, t);
  if (t == 0) p.bmax[(long)b * p.nblk + blockIdx.x] = mx;
}

__global__ __launch_bounds__(256) void fbank_norm_kernel(FbankP p) {
  __shared__ double red[4];
  const int t = threadIdx.x, m = blockIdx.x, b = blockIdx.y;
  const int n = row_len(p.lengths, b, p.T);
  const int nfr = 1 + n / DFT_HOP, nb = (nfr + DFT_FR - 1) / DFT_FR;
  double mx = -INFINITY;
  for (int i = t; i < nb; i += 256) mx = fmax(mx, p.bmax[(long)b * p.nblk + i]);
  const double floor_db = block_max<4>(mx, red, t) - 80.0;
  __syncthreads();                                                          // red is written again below
  const double* d = p.db + ((long)b * p.M + m) * p.F;
  double s = 0.0;
  for (int f = t; f < nfr; f += 256) s += fmax(d[f], floor_db);
  const double mean = block_sum_pairwise(s, red, t) / (double)nfr;
  float* o = p.out + b * p.o_bs + m * p.o_cs;
  for (int f = t; f < p.F; f += 256) o[f] = f < nfr ? (float)(fmax(d[f], floor_db) - mean) : 0.f;
  if (m == 0 && t == 0) p.frames[b] = nfr;
}

// ------------------------------------------------------------------------------------------------------------------- TDNN
struct TdnnP {
  int B, Cin, Cout, F, dil, epi;
  const float* x; long x_bs, x_cs;
  const float* x2; long x2_bs, x2_cs;
  const float* w; long w_rs;
  const float* bias; const float* row_bias; const float* scale; const float* shift;
  float* y; long y_bs, y_cs;
  const int* frames;
};

template <int K, int KC>
__global__ __launch_bounds__(TD_THREADS, 2) void tdnn_fwd_kernel(TdnnP p) {
  constexpr int WA = KC * K + 1;
  __shared__ float xs[KC * TD_XW];
  __shared__ float ws[TD_TM * WA];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = lane & 15, q = lane >> 4;
  const int b = blockIdx.z, t0 = blockIdx.x * TD_TN, co_blk = blockIdx.y * TD_TM;
  const int n = row_len(p.frames, b, p.F);
  if (t0 >= n) return;                                                      // uniform: frames at and past n are not written
  const int pad = (K - 1) * p.dil / 2, span = TD_TN + 2 * pad;              // pad <= 4: span <= 72 < TD_XW
  const int tend = min(t0 + TD_TN, n);
  const bool live = co_blk + 16 * w < p.Cout;                               // wave-uniform
  const float* xb = p.x + b * p.x_bs;
  const float* x2b = p.x2 ? p.x2 + b * p.x2_bs : nullptr;
  ec_f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = ec_f32x4{0.f, 0.f, 0.f, 0.f};
  // What this thread stages per chunk. XS inputs: element t + 256 s of xs is (channel c, column i) = ((t + 256 s) / 80, (t + 256 s)
  // % 80); 256 = 3 * 80 + 16, so the column repeats every 5 s and its source frame (which does not depend on the chunk; < 0: a zero)
  // is kept for s < 5 only. NW float4 of weights: float4 u = t + 256 s is row u / W4, columns 4 (u % W4) .. + 3 of the chunk's KC K.
  // The next chunk is loaded into registers before the MFMAs of this one and stored behind them.
  constexpr int XS = KC * TD_XW / TD_THREADS, W4 = KC * K / 4, NW = TD_TM * W4 / TD_THREADS;
  static_assert(KC * TD_XW % TD_THREADS == 0 && TD_TM * W4 % TD_THREADS == 0 && XS % 5 == 0, "staging shape");
  int src[5];
#pragma unroll
  for (int sl = 0; sl < 5; ++sl) {
    const int i = (t + TD_THREADS * sl) % TD_XW;
    int s = t0 - pad + i;
    src[sl] = -1;
    if (i < span && s < tend + pad) {                                       // a tap of an output frame below n
      if (s < 0) s = -s;
      if (s >= n) s = 2 * (n - 1) - s;
      src[sl] = min(max(s, 0), n - 1);                                      // n < pad + 1 (a row the definition refuses): stay inside the row
    }
  }
  const float* wrow[NW];
#pragma unroll
  for (int sl = 0; sl < NW; ++sl) {
    const int u = t + TD_THREADS * sl, r = u / W4;
    wrow[sl] = co_blk + r < p.Cout ? p.w + (long)(co_blk + r) * p.w_rs + 4 * (u - r * W4) : nullptr;
  }
  float xreg[XS];
  float4 wreg[NW];
  auto load = [&](int c0) {
#pragma unroll
    for (int sl = 0; sl < XS; ++sl) {
      const int c = c0 + (t + TD_THREADS * sl) / TD_XW, s = src[sl % 5];
      float v = 0.f;
      if (s >= 0 && c < p.Cin) {                                            // Cin is a multiple of 16, not always of KC
        v = xb[(long)c * p.x_cs + s];
        if (x2b) v += x2b[(long)c * p.x2_cs + s];
      }
      xreg[sl] = v;
    }
#pragma unroll
    for (int sl = 0; sl < NW; ++sl) {
      const int col = 4 * ((t + TD_THREADS * sl) % W4);                     // K (c0 + c) + tap < K Cin; both are multiples of 4
      wreg[sl] = wrow[sl] && c0 * K + col < p.Cin * K ? *reinterpret_cast<const float4*>(wrow[sl] + (long)c0 * K) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  load(0);
  for (int c0 = 0; c0 < p.Cin; c0 += KC) {
#pragma unroll
    for (int sl = 0; sl < XS; ++sl) xs[t + TD_THREADS * sl] = xreg[sl];
#pragma unroll
    for (int sl = 0; sl < NW; ++sl) {
      const int u = t + TD_THREADS * sl, r = u / W4;
      float* d = ws + r * WA + 4 * (u - r * W4);
      d[0] = wreg[sl].x; d[1] = wreg[sl].y; d[2] = wreg[sl].z; d[3] = wreg[sl].w;
    }
    __syncthreads();
    if (c0 + KC < p.Cin) load(c0 + KC);
    if (live) {
      ec_f32x4 part[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) part[nt] = ec_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KC / 4; ++kk)
#pragma unroll
        for (int tap = 0; tap < K; ++tap) {
          const float a = ws[(16 * w + j) * WA + (kk * 4 + q) * K + tap];
          const float* xr = xs + (kk * 4 + q) * TD_XW + tap * p.dil + j;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr[nt * 16], part[nt], 0, 0, 0);
        }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] += part[nt];
    }
    __syncthreads();
  }
  if (!live) return;
  float* yb = p.y + b * p.y_bs;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = co_blk + 16 * w + q * 4 + r;
    float add = p.bias ? p.bias[co] : 0.f;
    if (p.row_bias) add += p.row_bias[(long)b * p.Cout + co];
    const float sc = p.epi ? p.scale[co] : 1.f, sh = p.epi ? p.shift[co] : 0.f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int tt = t0 + nt * 16 + j;
      if (tt >= n) continue;
      float v = acc[nt][r] + add;
      if (p.epi) v = fmaf(fmaxf(v, 0.f), sc, sh);
      if (p.epi == 2) v = tanhf(v);
      yb[co * p.y_cs + tt] = v;
    }
  }
}

static int tdnn_check(const tdvc_tdnn_args* a, const char** why) {
  *why = nullptr;
  if (!a) { *why = "tdnn_fwd: null arguments"; return TDVC_EINVAL; }
  if (a->B < 0 || a->F < 0 || a->Cin < 1 || a->Cout < 1 || a->x_bs < 0 || a->x_cs < 0 || a->x2_bs < 0 || a->x2_cs < 0 || a->y_bs < 0 ||
      a->y_cs < 0 || a->w_rs < 0) { *why = "tdnn_fwd: negative size or stride"; return TDVC_EINVAL; }
  if (a->epilogue < 0 || a->epilogue > 2) { *why = "tdnn_fwd: epilogue must be 0 (none), 1 (ReLU, scale/shift) or 2 (that, tanh)"; return TDVC_EINVAL; }
  if (a->Cin % 16 || a->Cout % 16) { *why = "tdnn_fwd: channel counts must be multiples of 16"; return TDVC_EUNSUPPORTED; }
  if (a->K != 1 && a->K != 3 && a->K != 5) { *why = "tdnn_fwd: kernel size must be 1, 3 or 5"; return TDVC_EUNSUPPORTED; }
  if (a->dilation < 1 || a->dilation > 4) { *why = "tdnn_fwd: dilation must be 1..4"; return TDVC_EUNSUPPORTED; }
  if (a->F > 0 && a->F < 5) { *why = "tdnn_fwd: rows of fewer than 5 frames"; return TDVC_EUNSUPPORTED; }
  if (a->B > 65535 || a->Cout > (1 << 20) || a->Cin > (1 << 20) || a->F > (1 << 24)) { *why = "tdnn_fwd: B > 65535, more than 2^20 channels or 2^24 frames"; return TDVC_EUNSUPPORTED; }
  if (a->w_rs && (a->w_rs < (int64_t)a->Cin * a->K || a->w_rs % 4)) { *why = "tdnn_fwd: weight row stride below Cin K or not a multiple of 4"; return TDVC_EINVAL; }
  if (((uintptr_t)a->w & 15) != 0) { *why = "tdnn_fwd: weights must be 16-byte aligned"; return TDVC_EINVAL; }
  if (16 * a->x_cs + a->F > 0x7fffffffLL || 16 * a->x2_cs + a->F > 0x7fffffffLL) { *why = "tdnn_fwd: channel stride above 2^27"; return TDVC_EUNSUPPORTED; }
  if (a->B == 0 || a->F == 0) return TDVC_OK;
  if (!a->x || !a->w || !a->y || (a->epilogue && (!a->scale || !a->shift))) { *why = "tdnn_fwd: null pointer"; return TDVC_EINVAL; }
  return TDVC_OK;
}

static void tdnn_launch(const tdvc_tdnn_args* a, hipStream_t st) {
  TdnnP p;
  p.B = a->B; p.Cin = a->Cin; p.Cout = a->Cout; p.F = a->F; p.dil = a->dilation; p.epi = a->epilogue;
  p.x = a->x; p.x_bs = a->x_bs; p.x_cs = a->x_cs; p.x2 = a->x2; p.x2_bs = a->x2_bs; p.x2_cs = a->x2_cs;
  p.w = a->w; p.w_rs = a->w_rs ? a->w_rs : (long)a->Cin * a->K;
  p.bias = a->bias; p.row_bias = a->row_bias; p.scale = a->scale; p.shift = a->shift;
  p.y = a->y; p.y_bs = a->y_bs; p.y_cs = a->y_cs; p.frames = a->frames;
  const dim3 grid((a->F + TD_TN - 1) / TD_TN, (a->Cout + TD_TM - 1) / TD_TM, a->B);
  if (a->K == 1) hipLaunchKernelGGL((tdnn_fwd_kernel<1, 32>), grid, dim3(TD_THREADS), 0, st, p);
  else if (a->K == 3) hipLaunchKernelGGL((tdnn_fwd_kernel<3, 16>), grid, dim3(TD_THREADS), 0, st, p);
  else hipLaunchKernelGGL((tdnn_fwd_kernel<5, 16>), grid, dim3(TD_THREADS), 0, st, p);
}

// --------------------------------------------------------------------------------------------------------------------- SE
// gate is [B][C + S]: the means, then the gates, in the first C floats of a row, the hidden layer in the last S
__global__ __launch_bounds__(256) void se_mean_kernel(const float* x, long x_bs, long x_cs, int C, int S, int F, const int* frames, float* gate) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const int n = row_len(frames, b, F);
  const float* r = x + b * x_bs + c * x_cs;
  double s = 0.0;
  for (int f = lane; f < n; f += 64) s += (double)r[f];
  s = wave_sum(s);
  if (lane == 0) gate[(long)b * (C + S) + c] = n > 0 ? (float)(s / (double)n) : 0.f;
}

// a wave per output: out[o] = act(sum_i w[o][i] in[i] + bias[o]), relu (act 0) or sigmoid (act 1)
__global__ __launch_bounds__(256) void se_fc_kernel(float* gate, int stride, int in_off, int N, int out_off, const float* w, const float* bias, int act) {
  const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const float* in = gate + (long)b * stride + in_off;
  const float* wr = w + (long)o * N;
  double acc = 0.0;
  for (int i = lane; i < N; i += 64) acc = fma((double)wr[i], (double)in[i], acc);
  acc = wave_sum(acc) + (double)bias[o];
  if (lane == 0) gate[(long)b * stride + out_off + o] = act ? (float)(1.0 / (1.0 + exp(-acc))) : fmaxf((float)acc, 0.f);
}

__global__ __launch_bounds__(256) void se_apply_kernel(const float* x, long x_bs, long x_cs, const float* res, long r_bs, long r_cs, const float* gate,
                                                       int C, int S, int F, const int* frames, float* y, long y_bs, long y_cs) {
  const int f = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (f >= row_len(frames, b, F)) return;
  const float g = gate[(long)b * (C + S) + c];
  y[b * y_bs + c * y_cs + f] = fmaf(g, x[b * x_bs + c * x_cs + f], res[b * r_bs + c * r_cs + f]);
}

// -------------------------------------------------------------------------------------------------------------------- ASP
// wgt = null: uniform 1 / n (mask / total in speechbrain's _compute_statistics); else the softmax of lg over the row's frames
__global__ __launch_bounds__(256) void asp_stats_kernel(const float* x, long x_bs, long x_cs, const float* lg, int C, int F, const int* frames,
                                                        float* out) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const int n = row_len(frames, b, F);
  float* o = out + (long)b * 2 * C;
  if (n == 0) { if (lane == 0) { o[c] = 0.f; o[C + c] = 0.f; } return; }
  const float* r = x + b * x_bs + c * x_cs;
  const float* l = lg ? lg + ((long)b * C + c) * F : nullptr;
  double mx = -INFINITY, den = (double)n;
  if (l) {
    for (int f = lane; f < n; f += 64) mx = fmax(mx, (double)l[f]);
    mx = wave_max(mx);
    den = 0.0;
    for (int f = lane; f < n; f += 64) den += exp((double)l[f] - mx);
    den = wave_sum(den);
  }
  double m = 0.0;
  for (int f = lane; f < n; f += 64) m = fma(l ? exp((double)l[f] - mx) : 1.0, (double)r[f], m);
  m = wave_sum(m) / den;
  double v = 0.0;
  for (int f = lane; f < n; f += 64) {
    const double d = (double)r[f] - m;
    v = fma(l ? exp((double)l[f] - mx) : 1.0, d * d, v);
  }
  v = wave_sum(v) / den;
  if (lane == 0) { o[c] = (float)m; o[C + c] = (float)sqrt(fmax(v, 1e-12)); }
}

// rb[b][a] = sum_j W[a][C + j] ms[b][j], j < 2 C: the part of the 3 C -> A product whose input is constant over time
__global__ __launch_bounds__(256) void asp_rowbias_kernel(const float* w, const float* ms, int C, int A, float* rb) {
  const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const float* wr = w + (long)a * 3 * C + C;
  const float* m = ms + (long)b * 2 * C;
  double acc = 0.0;
  for (int jx = lane; jx < 2 * C; jx += 64) acc = fma((double)wr[jx], (double)m[jx], acc);
  acc = wave_sum(acc);
  if (lane == 0) rb[(long)b * A + a] = (float)acc;
}

__global__ __launch_bounds__(256) void ecapa_head_kernel(const float* pooled, const float* scale, const float* shift, const float* w, const float* bias,
                                                         int N, int E, float* out) {
  const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const float* pr = pooled + (long)b * N;
  const float* wr = w + (long)e * N;
  double acc = 0.0;
  for (int jx = lane; jx < N; jx += 64) acc = fma((double)wr[jx], (double)fmaf(pr[jx], scale[jx], shift[jx]), acc);
  acc = wave_sum(acc);
  if (lane == 0) out[(long)b * E + e] = (float)(acc + (double)bias[e]);
}

struct AspPlan { size_t ms, rb, h, lg, total; };
static bool asp_plan(int B, int C, int A, int F, AspPlan* pl) {
  if (B < 1 || C < 16 || A < 16 || F < 5 || C % 16 || A % 16 || B > 65535 || C > (1 << 20) || A > (1 << 20) || F > (1 << 24)) return false;
  if ((double)B * C * F > (double)(1L << 36)) return false;
  size_t off = 0;
  pl->ms = off; off += tdvc_align256((size_t)B * 2 * C * 4);
  pl->rb = off; off += tdvc_align256((size_t)B * A * 4);
  pl->h = off; off += tdvc_align256((size_t)B * A * F * 4);
  pl->lg = off; off += tdvc_align256((size_t)B * C * F * 4);
  pl->total = off;
  return true;
}

static bool fbank_ok(int B, int T, int M) { return B >= 1 && B <= 65535 && T >= 640 && T <= (1 << 26) && M >= 16 && M <= FB_MAXMEL && M % 16 == 0; }

}  // namespace tdvc

extern "C" size_t tdvc_fbank_workspace(int32_t B, int32_t T, int32_t n_mels) {
  using namespace tdvc;
  if (!fbank_ok(B, T, n_mels)) return 0;
  const size_t F = 1 + T / DFT_HOP, nblk = (F + DFT_FR - 1) / DFT_FR;
  return tdvc_align256((size_t)B * n_mels * F * 8) + tdvc_align256((size_t)B * nblk * 8);
}

extern "C" int tdvc_fbank(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, int32_t n_mels, const double* tables,
                          float* feats, int64_t f_bs, int64_t f_cs, int32_t F, int32_t* frames, void* workspace, size_t workspace_bytes,
                          void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || s_bs < 0 || f_bs < 0 || f_cs < 0) return tdvc_fail(TDVC_EINVAL, "fbank: negative B, T or stride");
  if (n_mels < 16 || n_mels > FB_MAXMEL || n_mels % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "fbank: n_mels must be a multiple of 16 up to 128");
  if (T < 640) return tdvc_fail(TDVC_EUNSUPPORTED, "fbank: rows of fewer than 640 samples (5 frames)");
  if (T > (1 << 26) || B > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "fbank: T > 2^26 or B > 65535");
  if (F != 1 + T / DFT_HOP) return tdvc_fail(TDVC_EINVAL, "fbank: F must be 1 + T / 160");
  if (f_cs < F) return tdvc_fail(TDVC_EINVAL, "fbank: band stride below F");
  if (B == 0) return TDVC_OK;
  if (!signal || !tables || !feats || !frames) return tdvc_fail(TDVC_EINVAL, "fbank: null pointer");
  const size_t need = tdvc_fbank_workspace(B, T, n_mels);
  if (!workspace || workspace_bytes < need) return tdvc_fail(TDVC_EWORKSPACE, "fbank: workspace too small (tdvc_fbank_workspace)");
  FbankP p;
  p.x = signal; p.x_bs = s_bs; p.lengths = lengths; p.T = T; p.F = F; p.M = n_mels; p.nblk = (F + DFT_FR - 1) / DFT_FR; p.tab = tables;
  p.db = (double*)workspace; p.bmax = (double*)((char*)workspace + tdvc_align256((size_t)B * n_mels * F * 8));
  p.out = feats; p.o_bs = f_bs; p.o_cs = f_cs; p.frames = frames;
  hipLaunchKernelGGL(fbank_db_kernel, dim3(p.nblk, B), dim3(256), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(fbank_norm_kernel, dim3(n_mels, B), dim3(256), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_tdnn_fwd(const tdvc_tdnn_args* a, void* stream) {
  using namespace tdvc;
  const char* why;
  const int rc = tdnn_check(a, &why);
  if (rc != TDVC_OK) return tdvc_fail(rc, why);
  if (a->B == 0 || a->F == 0) return TDVC_OK;
  tdnn_launch(a, (hipStream_t)stream);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_se_block(const float* x, int64_t x_bs, int64_t x_cs, const float* residual, int64_t r_bs, int64_t r_cs, int32_t B, int32_t C,
                             int32_t F, const int32_t* frames, int32_t S, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* gate, float* out, int64_t o_bs, int64_t o_cs, void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0 || C < 1 || S < 1 || x_bs < 0 || x_cs < 0 || r_bs < 0 || r_cs < 0 || o_bs < 0 || o_cs < 0)
    return tdvc_fail(TDVC_EINVAL, "se_block: negative size or stride");
  if (C % 16 || S % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "se_block: channel counts must be multiples of 16");
  if (C > SE_MAXC || S > SE_MAXC || B > 65535 || F > (1 << 24)) return tdvc_fail(TDVC_EUNSUPPORTED, "se_block: C or S > 65532, B > 65535 or F > 2^24");
  if (B == 0 || F == 0) return TDVC_OK;
  if (!x || !residual || !w1 || !b1 || !w2 || !b2 || !gate || !out) return tdvc_fail(TDVC_EINVAL, "se_block: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(se_mean_kernel, dim3(C / 4, B), dim3(256), 0, st, x, (long)x_bs, (long)x_cs, C, S, F, frames, gate);
  hipLaunchKernelGGL(se_fc_kernel, dim3(S / 4, B), dim3(256), 0, st, gate, C + S, 0, C, C, w1, b1, 0);
  hipLaunchKernelGGL(se_fc_kernel, dim3(C / 4, B), dim3(256), 0, st, gate, C + S, C, S, 0, w2, b2, 1);
  hipLaunchKernelGGL(se_apply_kernel, dim3((F + 255) / 256, C, B), dim3(256), 0, st, x, (long)x_bs, (long)x_cs, residual, (long)r_bs, (long)r_cs,
                     (const float*)gate, C, S, F, frames, out, (long)o_bs, (long)o_cs);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" size_t tdvc_asp_pool_workspace(int32_t B, int32_t C, int32_t A, int32_t F) {
  tdvc::AspPlan pl;
  return tdvc::asp_plan(B, C, A, F, &pl) ? pl.total : 0;
}

extern "C" int tdvc_asp_pool(const float* x, int64_t x_bs, int64_t x_cs, int32_t B, int32_t C, int32_t F, const int32_t* frames, int32_t A,
                             const float* w_tdnn, const float* b_tdnn, const float* scale, const float* shift, const float* w_conv,
                             const float* b_conv, float* pooled, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0 || C < 1 || A < 1 || x_bs < 0 || x_cs < 0) return tdvc_fail(TDVC_EINVAL, "asp_pool: negative size or stride");
  if (C % 16 || A % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "asp_pool: channel counts must be multiples of 16");
  if (F > 0 && F < 5) return tdvc_fail(TDVC_EUNSUPPORTED, "asp_pool: rows of fewer than 5 frames");
  if (B == 0 || F == 0) return TDVC_OK;
  AspPlan pl;
  if (!asp_plan(B, C, A, F, &pl)) return tdvc_fail(TDVC_EUNSUPPORTED, "asp_pool: B > 65535, more than 2^20 channels, 2^24 frames or 2^36 elements");
  if (!x || !w_tdnn || !b_tdnn || !scale || !shift || !w_conv || !b_conv || !pooled) return tdvc_fail(TDVC_EINVAL, "asp_pool: null pointer");
  if ((((uintptr_t)w_tdnn | (uintptr_t)w_conv) & 15) != 0) return tdvc_fail(TDVC_EINVAL, "asp_pool: weights must be 16-byte aligned");
  if (16 * x_cs + F > 0x7fffffffLL) return tdvc_fail(TDVC_EUNSUPPORTED, "asp_pool: channel stride above 2^27");
  if (!workspace || workspace_bytes < pl.total) return tdvc_fail(TDVC_EWORKSPACE, "asp_pool: workspace too small (tdvc_asp_pool_workspace)");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ms = (float*)(ws + pl.ms);
  float* rb = (float*)(ws + pl.rb);
  float* h = (float*)(ws + pl.h);
  float* lg = (float*)(ws + pl.lg);
  hipLaunchKernelGGL(asp_stats_kernel, dim3(C / 4, B), dim3(256), 0, st, x, (long)x_bs, (long)x_cs, (const float*)nullptr, C, F, frames, ms);
  hipLaunchKernelGGL(asp_rowbias_kernel, dim3(A / 4, B), dim3(256), 0, st, w_tdnn, (const float*)ms, C, A, rb);
  tdvc_tdnn_args a = {};
  a.B = B; a.Cin = C; a.Cout = A; a.F = F; a.K = 1; a.dilation = 1; a.epilogue = 2;
  a.x = x; a.x_bs = x_bs; a.x_cs = x_cs; a.w = w_tdnn; a.w_rs = (int64_t)3 * C; a.bias = b_tdnn; a.row_bias = rb; a.scale = scale; a.shift = shift;
  a.y = h; a.y_bs = (int64_t)A * F; a.y_cs = F; a.frames = frames;
  tdnn_launch(&a, st);
  tdvc_tdnn_args c = {};
  c.B = B; c.Cin = A; c.Cout = C; c.F = F; c.K = 1; c.dilation = 1; c.epilogue = 0;
  c.x = h; c.x_bs = (int64_t)A * F; c.x_cs = F; c.w = w_conv; c.bias = b_conv; c.y = lg; c.y_bs = (int64_t)C * F; c.y_cs = F; c.frames = frames;
  tdnn_launch(&c, st);
  hipLaunchKernelGGL(asp_stats_kernel, dim3(C / 4, B), dim3(256), 0, st, x, (long)x_bs, (long)x_cs, (const float*)lg, C, F, frames, pooled);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_ecapa_head(const float* pooled, int32_t B, int32_t N, const float* scale, const float* shift, const float* w, const float* bias,
                               int32_t E, float* emb, void* stream) {
  using namespace tdvc;
  if (B < 0 || N < 1 || E < 1) return tdvc_fail(TDVC_EINVAL, "ecapa_head: negative B, N or E < 1");
  if (N % 16 || E % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "ecapa_head: channel counts must be multiples of 16");
  if (B > 65535 || N > (1 << 24) || E > (1 << 20)) return tdvc_fail(TDVC_EUNSUPPORTED, "ecapa_head: B > 65535, N > 2^24 or E > 2^20");
  if (B == 0) return TDVC_OK;
  if (!pooled || !scale || !shift || !w || !bias || !emb) return tdvc_fail(TDVC_EINVAL, "ecapa_head: null pointer");
  hipLaunchKernelGGL(ecapa_head_kernel, dim3(E / 4, B), dim3(256), 0, (hipStream_t)stream, pooled, scale, shift, w, bias, N, E, emb);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
