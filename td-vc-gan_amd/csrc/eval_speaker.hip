// Speaker-similarity evaluation (the live path of the reference's test_scripts/common/test_speaker_rec.py: Resemblyzer's
// VoiceEncoder.embed_utterance), restated in include/tdvc.h: a 40-band mel power spectrogram, a 3-layer LSTM of 256 units over
// overlapping windows of 160 frames, linear + ReLU + L2 norm, the mean over the windows.
//
// tdvc_voice_windows   one thread per row: window count, (row, start frame) per slot, from the device lengths
// tdvc_voice_gain      one block per row: sum of squares in float64, fixed order -> the volume gain of normalize=True
// tdvc_voice_mel       one block per 8 frames of a row: the padded-row index mapping, Hann window, a direct 400-point float64 DFT
//                      against a cos/sin table of 400 entries held in LDS (index k i mod 400), power (that stage: dft400.h), the 40
//                      mel sums in float64, one rounding at the store
// tdvc_lstm_fwd        per layer: pack W_ih / W_hh into the MFMA operand order (lstm_pack_kernel), the input projection of every
//                      frame as one GEMM (lstm_proj_kernel), then the recurrence (lstm_rec_kernel)
// tdvc_voice_embed     one block per row: linear + ReLU + L2 norm per window, the mean over the row's windows, the second norm
//
// The recurrence. One workgroup of 512 threads (8 waves) owns a tile of 16 windows for all steps of a layer; blocks never wait
// for one another (layers are separated by stream order), so no spin-wait can hang the device. Per step the tile needs
// G[16][1024] = h[16][256] W_hh^T on v_mfma_f32_16x16x4_f32 (exact fp32). Wave w owns the hidden units [32 w, 32 w + 32) and
// eight accumulator tiles, gate (i, f, g, o) x two blocks of 16 units, whose column j is W_hh's row gate * 256 + 32 w + 16 cb + j:
// a lane therefore holds the four gate pre-activations of 8 (window, unit) pairs and keeps their cell state c in 8 registers, and
// the cell update needs no exchange. h is double-buffered in LDS (2 x 16 x 260 floats): a step reads buffer `cur` as the A
// operand, writes h' into the other one, and one barrier separates the steps. The MFMA's four k slots are given to the four
// quarters of the reduction (lanes 16 q .. 16 q + 15 take k in [q K/4, (q + 1) K/4)), so that a lane reads four consecutive k as
// one ds_read_b128 / one global_load_dwordx4; the weights are packed once per call so that each such load is 1 KB contiguous per
// wave. W_hh is 1 MB: it does not fit the CU and is streamed from L2 every step. The MFMA work of a step is
// 2 * 16 * 1024 * 256 flop at 64 flop/clk/SIMD = 32768 cycles (13.7 us), against 1 MB at 64 B/clk from L2 = 16384.
// The tile is 16 windows and not the 32 of v_mfma_f32_32x32x2_f32 because the step time is the MFMA time of one compute unit,
// which is proportional to the tile's rows, and an evaluation set has far fewer tiles than the device has compute units:
// measured 19.6 ms with 32-row tiles against 11.2 ms with 16-row tiles for 80 windows (profiles/speaker_bench.txt, DESIGN.md
// section 3).
// The input projection x_t W_ih^T + b_ih + b_hh is hoisted out of the time loop; layer 0 projects every frame of an
// utterance once, not once per overlapping window. Its result initialises the accumulators of the step.
// No atomics anywhere; every sum has a fixed order (block sums: the pairwise order of reduce.h): bit-identical from call to call.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include "dft400.h"
#include "reduce.h"

namespace tdvc {

constexpr int VM_MELS = 40, VM_WIN = 160;                                               // window of 160 frames = 25600 samples
constexpr int LS_H = 256, LS_G = 4 * LS_H, LS_M = 16, LS_LDA = LS_H + 4, LS_THREADS = 512;

// compute_partial_slices in closed form: the number of kept windows of a row of n samples and its padded length L'.
__host__ __device__ inline int vw_count(long n, int frame_step, double min_cov, long* padded) {
  const long n_frames = (n + 1 + DFT_HOP - 1) / DFT_HOP;
  long steps = n_frames - VM_WIN + frame_step + 1;
  if (steps < 1) steps = 1;
  long cnt = (steps + frame_step - 1) / frame_step;
  if (cnt > 1) {
    const long first = (long)DFT_HOP * (cnt - 1) * frame_step;
    if ((double)(n - first) / (double)(DFT_HOP * VM_WIN) < min_cov) --cnt;
  }
  const long end = (long)DFT_HOP * ((cnt - 1) * frame_step + VM_WIN);
  if (padded) *padded = n > end ? n : end;
  return (int)cnt;
}

__global__ __launch_bounds__(256) void voice_windows_kernel(const int* lengths, int T, int B, int frame_step, double min_cov, int P_max,
                                                            int* counts, int* slots) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int n = row_len(lengths, b, T);
  const int cnt = min(vw_count(n, frame_step, min_cov, nullptr), P_max);
  counts[b] = cnt;
  for (int j = 0; j < P_max; ++j) {
    slots[2 * ((long)b * P_max + j)] = b;
    slots[2 * ((long)b * P_max + j) + 1] = j * frame_step;
  }
}

__global__ __launch_bounds__(256) void voice_gain_kernel(const float* x, long x_bs, const int* lengths, int T, double* gain) {
  __shared__ double red[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = row_len(lengths, b, T);
  const float* row = x + b * x_bs;
  double acc = 0.0;
  for (int i = t; i < n; i += 256) { const double v = (double)row[i]; acc = fma(v, v, acc); }
  block_stage(wave_sum(acc), red, t);
  if (t == 0) {
    const double ss = (red[0] + red[1]) + (red[2] + red[3]);     // sum_pairwise, spelled out: as a call the branch below compiles differently
    double g = 1.0;
    if (n > 0 && ss > 0.0) {
      const double rms = sqrt(ss / (double)n);
      g = pow(10.0, (-30.0 - 20.0 * log10(rms)) / 20.0);
      if (!(g > 1.0)) g = 1.0;                                              // increase_only
    }
    gain[b] = g;
  }
}

struct MelP {
  const float* x; long x_bs;
  const int* lengths; int T, F, frame_step; double min_cov; int pad_const;
  const double* gain;
  const double* tab;      // cos[400], sin[400], hann[400], fb[40][201]
  float* out;
};

__global__ __launch_bounds__(256) void voice_mel_kernel(MelP p) {
  __shared__ double cs[2 * DFT_NFFT];
  __shared__ double xw[DFT_FR][DFT_NFFT];
  __shared__ double pw[DFT_FR][DFT_BINS];
  const int t = threadIdx.x, b = blockIdx.y;
  const int f0 = blockIdx.x * DFT_FR;
  const int n = row_len(p.lengths, b, p.T);
  long Lp;
  vw_count(n, p.frame_step, p.min_cov, &Lp);
  const long nfr = 1 + Lp / DFT_HOP;
  const double g = p.gain ? p.gain[b] : 1.0;
  const float* row = p.x + b * p.x_bs;
  for (int i = t; i < 2 * DFT_NFFT; i += 256) cs[i] = p.tab[i];
  for (int idx = t; idx < DFT_FR * DFT_NFFT; idx += 256) {
    const int fr = idx / DFT_NFFT, i = idx - fr * DFT_NFFT;
    const long f = f0 + fr;
    double v = 0.0;
    if (f < nfr) {
      long q = f * DFT_HOP - DFT_NFFT / 2 + i;
      if (!p.pad_const) {                                                   // L' >= 25600: one reflection reaches every index
        if (q < 0) q = -q;
        if (q >= Lp) q = 2 * (Lp - 1) - q;
      }
      if (q >= 0 && q < n) v = (double)row[q] * g * p.tab[DFT_TAB_WINDOW + i];
    }
    xw[fr][i] = v;
  }
  __syncthreads();
  dft400_power<256>(cs, xw, pw, t);
  __syncthreads();
  const double* fb = p.tab + DFT_TAB_FB;
  for (int item = t; item < DFT_FR * VM_MELS; item += 256) {
    const int fr = item / VM_MELS, m = item - fr * VM_MELS;
    const long f = f0 + fr;
    if (f >= p.F) continue;
    double acc = 0.0;
    if (f < nfr)
      for (int k = 0; k < DFT_BINS; ++k) acc = fma(fb[m * DFT_BINS + k], pw[fr][k], acc);
    p.out[((long)b * p.F + f) * VM_MELS + m] = (float)acc;
  }
}

// ------------------------------------------------------------------------------------------------------------------ LSTM
typedef float f32x4 __attribute__((ext_vector_type(4)));

// A lane of a wave is (j = lane & 15, q = lane >> 4): row j of the A tile and column j of a B tile, and the q-th quarter of the
// reduction, which is the MFMA's k slot. Wave w owns the hidden units [32 w, 32 w + 32) as 8 tiles tl = 2 gate + cb of 16 columns,
// column j of tile tl being the weight row gate * 256 + 32 w + 16 cb + j.
// W [1024][K] row-major -> packed [wave 8][kk4 Kp/16][tile 8][lane 64] float4, Kp = K rounded up to 16 (zeros behind K):
// the lane's float4 is W[that row][q Kp/4 + 4 kk4 .. + 3]
__global__ __launch_bounds__(256) void lstm_pack_kernel(const float* W, int K, int Kp, float4* out) {
  const int nk4 = Kp / 16, quarter = Kp / 4;
  const long total = (long)8 * nk4 * 8 * 64;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int lane = (int)(idx & 63), tl = (int)((idx >> 6) & 7);
    const int kk4 = (int)((idx >> 9) % nk4), wave = (int)((idx >> 9) / nk4);
    const int j = lane & 15, q = lane >> 4;
    const float* r = W + (long)((tl >> 1) * LS_H + 32 * wave + 16 * (tl & 1) + j) * K;
    const int k0 = q * quarter + 4 * kk4;
    float4 v;
    v.x = k0 + 0 < K ? r[k0 + 0] : 0.f;
    v.y = k0 + 1 < K ? r[k0 + 1] : 0.f;
    v.z = k0 + 2 < K ? r[k0 + 2] : 0.f;
    v.w = k0 + 3 < K ? r[k0 + 3] : 0.f;
    out[idx] = v;
  }
}

// acc[tile] += four consecutive k of A (LDS, this lane's row and quarter: a) times the packed weights (this wave's and lane's: bp);
// consecutive MFMAs go to different accumulators
__device__ __forceinline__ void lstm_mma4(f32x4 (&acc)[8], const float* a, const float4* bp, int kk4) {
  const float4 av = *reinterpret_cast<const float4*>(a + 4 * kk4);
  float4 bv[8];
#pragma unroll
  for (int tl = 0; tl < 8; ++tl) bv[tl] = bp[(kk4 * 8 + tl) * 64];
#pragma unroll
  for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[tl].x, acc[tl], 0, 0, 0);
#pragma unroll
  for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[tl].y, acc[tl], 0, 0, 0);
#pragma unroll
  for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[tl].z, acc[tl], 0, 0, 0);
#pragma unroll
  for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[tl].w, acc[tl], 0, 0, 0);
}

// acc += A W^T over nk4 groups of 16 k, in chunks of 64 k (16 dependent MFMAs per accumulator), each summed from zero and then
// added: with one chain over all of K the rounding of the running sum dominated the error of a one-step run (measured with
// 32-row tiles: 1.3 of the test's bar of 4 x the fp32 CPU error; 0.31 with the chunks)
__device__ __forceinline__ void lstm_gemm(f32x4 (&acc)[8], const float* a, const float4* bp, int nk4) {
#pragma unroll 1
  for (int k0 = 0; k0 < nk4; k0 += 4) {
    f32x4 part[8];
#pragma unroll
    for (int tl = 0; tl < 8; ++tl) part[tl] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int k1 = min(k0 + 4, nk4);
    for (int kk4 = k0; kk4 < k1; ++kk4) lstm_mma4(part, a, bp, kk4);
#pragma unroll
    for (int tl = 0; tl < 8; ++tl) acc[tl] += part[tl];
  }
}

struct ProjP {
  const float* x; long x_bs, x_fs; int F;      // row r of the GEMM is x + (r / F) x_bs + (r % F) x_fs
  long NR; int K, Kp;
  const float4* wp; const float* b_ih; const float* b_hh;
  float* out;                                   // [NR][1024]
};

__global__ __launch_bounds__(LS_THREADS) void lstm_proj_kernel(ProjP p) {
  __shared__ __attribute__((aligned(16))) float A[LS_M * LS_LDA];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = lane & 15, q = lane >> 4;
  const long r0 = (long)blockIdx.x * LS_M;
  for (int idx = t; idx < LS_M * p.Kp; idx += LS_THREADS) {
    const int i = idx / p.Kp, k = idx - i * p.Kp;
    const long r = r0 + i;
    float v = 0.f;
    if (r < p.NR && k < p.K) v = p.x[(r / p.F) * p.x_bs + (r % p.F) * p.x_fs + k];
    A[i * LS_LDA + k] = v;
  }
  __syncthreads();
  f32x4 acc[8];
#pragma unroll
  for (int tl = 0; tl < 8; ++tl) {
    const int col = (tl >> 1) * LS_H + 32 * w + 16 * (tl & 1) + j;
    const float bias = p.b_ih[col] + p.b_hh[col];
    acc[tl] = f32x4{bias, bias, bias, bias};
  }
  const int nk4 = p.Kp / 16;
  lstm_gemm(acc, A + j * LS_LDA + q * (p.Kp / 4), p.wp + (long)w * nk4 * 512 + lane, nk4);
#pragma unroll
  for (int tl = 0; tl < 8; ++tl)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = r0 + q * 4 + r;
      if (row < p.NR) p.out[row * LS_G + (tl >> 1) * LS_H + 32 * w + 16 * (tl & 1) + j] = acc[tl][r];
    }
}

struct RecP {
  const float* xp;              // projected inputs [rows][1024]
  int per_slot;                 // 0: row of slot = slot_row * F + start (layer 0); 1: slot * T_steps
  const int* slots; const int* counts;
  int P, P_max, B, F, T_steps;
  const float4* wp;             // packed W_hh
  float* hseq;                  // [P][T_steps][256] or null
  float* h_out;                 // [P][256] or null: h after the last step, zero for unused slots
};

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(LS_THREADS) void lstm_rec_kernel(RecP p) {
  __shared__ __attribute__((aligned(16))) float hb[2][LS_M * LS_LDA];
  __shared__ int xb_s[LS_M];
  __shared__ int any_s;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = lane & 15, q = lane >> 4;
  const int slot0 = blockIdx.x * LS_M;
  if (t == 0) any_s = 0;
  __syncthreads();
  if (t < LS_M) {
    const int slot = slot0 + t;
    int xb = -1;
    if (slot < p.P) {
      const int row = p.slots[2 * slot], start = p.slots[2 * slot + 1];
      bool ok = row >= 0 && row < p.B && start >= 0 && (long)start + p.T_steps <= p.F;
      if (ok && p.counts) ok = (slot % p.P_max) < p.counts[row];
      if (ok) xb = p.per_slot ? slot * p.T_steps : row * p.F + start;
    }
    xb_s[t] = xb;
    if (xb >= 0) any_s = 1;                                                 // every writer stores the same value
  }
  for (int i = t; i < LS_M * LS_LDA; i += LS_THREADS) hb[0][i] = 0.f;
  __syncthreads();
  if (!any_s) {                                                             // uniform: a tile of unused slots
    if (p.h_out)
      for (int i = t; i < LS_M * LS_H; i += LS_THREADS)
        if (slot0 + i / LS_H < p.P) p.h_out[(long)slot0 * LS_H + i] = 0.f;
    return;
  }
  // this lane's cells: windows q * 4 + r, r < 4, units 32 w + 16 cb + j, cb < 2. A used slot exists, so the rows 0 .. T_steps - 1
  // of xp exist: an unused window reads them (and discards what it read) rather than branching around the load
  int xb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xb[r] = xb_s[q * 4 + r];
  float c[2][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) c[0][r] = c[1][r] = 0.f;
  const float4* bp = p.wp + (long)w * (LS_H / 16) * 512 + lane;
  const int u0 = 32 * w + j;
  int cur = 0;
  for (int step = 0; step < p.T_steps; ++step) {
    f32x4 acc[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* xr = p.xp + ((long)max(xb[r], 0) + step) * LS_G + u0;
#pragma unroll
      for (int tl = 0; tl < 8; ++tl) {
        const float v = xr[(tl >> 1) * LS_H + 16 * (tl & 1)];
        acc[tl][r] = xb[r] >= 0 ? v : 0.f;
      }
    }
    lstm_gemm(acc, hb[cur] + j * LS_LDA + q * (LS_H / 4), bp, LS_H / 16);
    float* hn = hb[cur ^ 1];
    const bool last = step == p.T_steps - 1;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q * 4 + r, u = u0 + 16 * cb;
        const float ig = lstm_sigmoid(acc[0 + cb][r]), fg = lstm_sigmoid(acc[2 + cb][r]), gg = tanhf(acc[4 + cb][r]),
                    og = lstm_sigmoid(acc[6 + cb][r]);
        c[cb][r] = fg * c[cb][r] + ig * gg;
        const float hv = og * tanhf(c[cb][r]);
        hn[i * LS_LDA + u] = hv;
        const int slot = slot0 + i;
        if (p.hseq && xb[r] >= 0) p.hseq[((long)slot * p.T_steps + step) * LS_H + u] = hv;
        if (last && p.h_out && slot < p.P) p.h_out[(long)slot * LS_H + u] = xb[r] >= 0 ? hv : 0.f;
      }
    __syncthreads();
    cur ^= 1;
  }
}

struct EmbP {
  const float* h; int P_max; const int* counts;
  const float* W; const float* bias;
  float* partial; float* utt;
};

__global__ __launch_bounds__(256) void voice_embed_kernel(EmbP p) {
  __shared__ float hs[LS_H], e[LS_H], red[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x;
  const int cnt = p.counts ? min(max(p.counts[b], 0), p.P_max) : p.P_max;
  float sum = 0.f;
  for (int jw = 0; jw < p.P_max; ++jw) {
    const long slot = (long)b * p.P_max + jw;
    if (jw >= cnt) {
      if (p.partial) p.partial[slot * LS_H + t] = 0.f;
      continue;
    }
    hs[t] = p.h[slot * LS_H + t];
    __syncthreads();
    for (int o = wv * 64; o < wv * 64 + 64; ++o) {
      const float* wr = p.W + (long)o * LS_H;
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) acc = fmaf(wr[lane + 64 * m], hs[lane + 64 * m], acc);
      acc = wave_sum(acc);
      if (lane == 0) e[o] = fmaxf(acc + p.bias[o], 0.f);
    }
    __syncthreads();
    const float v = e[t];
    const float ss = block_sum_pairwise(v * v, red, t);
    __syncthreads();                                                        // red is written again below
    const float en = v / sqrtf(ss);                                         // no epsilon: an all-zero e gives NaN, as the reference
    if (p.partial) p.partial[slot * LS_H + t] = en;
    sum += en;
  }
  if (p.utt) {
    const float m = sum / (float)cnt;
    const float ss = block_sum_pairwise(m * m, red, t);
    __syncthreads();
    p.utt[(long)b * LS_H + t] = m / sqrtf(ss);
  }
}

static inline int ls_kp(int K) { return (K + 15) & ~15; }

struct LstmPlan { size_t wih[3], whh[3], xp, hseq, total; long rows0, rowsN; };

static bool lstm_plan(int B, int F, int I, int P, int T_steps, int layers, LstmPlan* pl) {
  if (B < 1 || F < 1 || P < 1 || I < 1 || I > LS_H || layers < 1 || layers > 3 || T_steps < 1 || T_steps > VM_WIN) return false;
  pl->rows0 = (long)B * F; pl->rowsN = (long)P * T_steps;
  if (pl->rows0 > (1L << 21) || pl->rowsN > (1L << 21)) return false;
  size_t off = 0;
  for (int l = 0; l < layers; ++l) {
    pl->wih[l] = off; off += tdvc_align256((size_t)LS_G * ls_kp(l ? LS_H : I) * 4);
    pl->whh[l] = off; off += tdvc_align256((size_t)LS_G * LS_H * 4);
  }
  const long rows = layers > 1 && pl->rowsN > pl->rows0 ? pl->rowsN : pl->rows0;
  pl->xp = off; off += tdvc_align256((size_t)rows * LS_G * 4);
  pl->hseq = off; off += layers > 1 ? tdvc_align256((size_t)pl->rowsN * LS_H * 4) : 0;
  pl->total = off;
  return true;
}

}  // namespace tdvc

extern "C" int32_t tdvc_voice_window_count(int64_t n, int32_t frame_step, double min_coverage, int64_t* padded) {
  if (n < 0 || n > 0x7fffffff || frame_step < 1 || frame_step > (1 << 20)) { if (padded) *padded = 0; return 0; }
  long lp = 0;
  const int c = tdvc::vw_count((long)n, frame_step, min_coverage, &lp);
  if (padded) *padded = lp;
  return c;
}

extern "C" int tdvc_voice_windows(const int32_t* lengths, int32_t T, int32_t B, int32_t frame_step, double min_coverage, int32_t P_max,
                                  int32_t* counts, int32_t* slots, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || P_max < 1 || frame_step < 1) return tdvc_fail(TDVC_EINVAL, "voice_windows: negative B or T, P_max or frame_step < 1");
  if (!(min_coverage == min_coverage)) return tdvc_fail(TDVC_EINVAL, "voice_windows: min_coverage is NaN");
  if (T > (1 << 26) || frame_step > (1 << 20) || (int64_t)B * P_max > (1 << 24))
    return tdvc_fail(TDVC_EUNSUPPORTED, "voice_windows: T > 2^26, frame_step > 2^20 or more than 2^24 slots");
  if (B == 0) return TDVC_OK;
  if (!counts || !slots) return tdvc_fail(TDVC_EINVAL, "voice_windows: null pointer");
  hipLaunchKernelGGL(voice_windows_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, lengths, T, B, frame_step, min_coverage,
                     P_max, counts, slots);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_voice_gain(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, double* gain, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || s_bs < 0) return tdvc_fail(TDVC_EINVAL, "voice_gain: negative B, T or stride");
  if (B > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "voice_gain: B > 65535");
  if (B == 0) return TDVC_OK;
  if (!gain || (!signal && T > 0)) return tdvc_fail(TDVC_EINVAL, "voice_gain: null pointer");
  hipLaunchKernelGGL(voice_gain_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, signal, (long)s_bs, lengths, T, gain);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_voice_mel(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, int32_t F, int32_t frame_step,
                              double min_coverage, int32_t pad_constant, const double* gain, const double* tables, float* mel, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || F < 0 || s_bs < 0 || frame_step < 1) return tdvc_fail(TDVC_EINVAL, "voice_mel: negative B, T, F or stride, frame_step < 1");
  if (!(min_coverage == min_coverage)) return tdvc_fail(TDVC_EINVAL, "voice_mel: min_coverage is NaN");
  if (!pad_constant && T <= DFT_NFFT / 2) return tdvc_fail(TDVC_EUNSUPPORTED, "voice_mel: reflect padding needs T > 200 samples");
  if (T > (1 << 26) || frame_step > (1 << 20) || B > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "voice_mel: T > 2^26, frame_step > 2^20 or B > 65535");
  if (B == 0 || F == 0) return TDVC_OK;
  if (!signal || !tables || !mel) return tdvc_fail(TDVC_EINVAL, "voice_mel: null pointer");
  MelP p;
  p.x = signal; p.x_bs = s_bs; p.lengths = lengths; p.T = T; p.F = F; p.frame_step = frame_step; p.min_cov = min_coverage;
  p.pad_const = pad_constant; p.gain = gain; p.tab = tables; p.out = mel;
  hipLaunchKernelGGL(voice_mel_kernel, dim3((F + DFT_FR - 1) / DFT_FR, B), dim3(256), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" size_t tdvc_lstm_workspace(int32_t B, int32_t F, int32_t I, int32_t P, int32_t T_steps, int32_t layers) {
  tdvc::LstmPlan pl;
  return tdvc::lstm_plan(B, F, I, P, T_steps, layers, &pl) ? pl.total : 0;
}

extern "C" int tdvc_lstm_fwd(const float* frames, int64_t f_bs, int64_t f_fs, int32_t B, int32_t F, int32_t I, const int32_t* slots,
                             const int32_t* counts, int32_t P, int32_t P_max, int32_t T_steps, int32_t layers, const float* const* weights,
                             float* h_out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0 || P < 0 || f_bs < 0 || f_fs < 0) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: negative B, F, P or stride");
  if (I < 1) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: input size < 1");
  if (I > LS_H) return tdvc_fail(TDVC_EUNSUPPORTED, "lstm_fwd: input size above 256");
  if (layers < 1 || layers > 3) return tdvc_fail(TDVC_EUNSUPPORTED, "lstm_fwd: 1 to 3 layers");
  if (T_steps < 1 || T_steps > VM_WIN) return tdvc_fail(TDVC_EUNSUPPORTED, "lstm_fwd: 1 to 160 steps");
  if (counts && P_max < 1) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: counts need P_max >= 1");
  if (F > 1 && f_fs < I) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: frame stride below the input size");
  if (P == 0) return TDVC_OK;
  if (B == 0 || F == 0) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: windows of an empty frame array");
  LstmPlan pl;
  if (!lstm_plan(B, F, I, P, T_steps, layers, &pl)) return tdvc_fail(TDVC_EUNSUPPORTED, "lstm_fwd: more than 2^21 frames or window steps");
  if (!frames || !slots || !weights || !h_out) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: null pointer");
  for (int i = 0; i < 4 * layers; ++i)
    if (!weights[i]) return tdvc_fail(TDVC_EINVAL, "lstm_fwd: null weight pointer");
  if (!workspace || workspace_bytes < pl.total) return tdvc_fail(TDVC_EWORKSPACE, "lstm_fwd: workspace too small (tdvc_lstm_workspace)");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* xp = (float*)(ws + pl.xp);
  float* hseq = layers > 1 ? (float*)(ws + pl.hseq) : nullptr;
  const int tiles = (P + LS_M - 1) / LS_M;
  for (int l = 0; l < layers; ++l) {
    const int K = l ? LS_H : I, Kp = ls_kp(K);
    float4* wih = (float4*)(ws + pl.wih[l]);
    float4* whh = (float4*)(ws + pl.whh[l]);
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(Kp), dim3(256), 0, st, weights[4 * l], K, Kp, wih);
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(LS_H), dim3(256), 0, st, weights[4 * l + 1], LS_H, LS_H, whh);
    ProjP pp;
    if (l == 0) { pp.x = frames; pp.x_bs = f_bs; pp.x_fs = f_fs; pp.F = F; pp.NR = pl.rows0; }
    else { pp.x = hseq; pp.x_bs = 0; pp.x_fs = LS_H; pp.F = 0x7fffffff; pp.NR = pl.rowsN; }
    pp.K = K; pp.Kp = Kp; pp.wp = wih; pp.b_ih = weights[4 * l + 2]; pp.b_hh = weights[4 * l + 3]; pp.out = xp;
    hipLaunchKernelGGL(lstm_proj_kernel, dim3((unsigned)((pp.NR + LS_M - 1) / LS_M)), dim3(LS_THREADS), 0, st, pp);
    RecP rp;
    rp.xp = xp; rp.per_slot = l > 0; rp.slots = slots; rp.counts = counts; rp.P = P; rp.P_max = P_max > 0 ? P_max : 1; rp.B = B; rp.F = F;
    rp.T_steps = T_steps; rp.wp = whh; rp.hseq = l + 1 < layers ? hseq : nullptr; rp.h_out = l + 1 == layers ? h_out : nullptr;
    hipLaunchKernelGGL(lstm_rec_kernel, dim3(tiles), dim3(LS_THREADS), 0, st, rp);
  }
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_voice_embed(const float* h, int32_t B, int32_t P_max, const int32_t* counts, const float* W, const float* bias,
                                float* partial, float* utt, void* stream) {
  using namespace tdvc;
  if (B < 0 || P_max < 1) return tdvc_fail(TDVC_EINVAL, "voice_embed: negative B or P_max < 1");
  if ((int64_t)B * P_max > (1 << 24)) return tdvc_fail(TDVC_EUNSUPPORTED, "voice_embed: more than 2^24 slots");
  if (B == 0) return TDVC_OK;
  if (!h || !W || !bias || (!partial && !utt)) return tdvc_fail(TDVC_EINVAL, "voice_embed: null pointer");
  EmbP p;
  p.h = h; p.P_max = P_max; p.counts = counts; p.W = W; p.bias = bias; p.partial = partial; p.utt = utt;
  hipLaunchKernelGGL(voice_embed_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
