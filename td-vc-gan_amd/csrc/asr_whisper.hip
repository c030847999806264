// The Whisper ASR metric (HF WhisperForConditionalGeneration in eval mode plus WhisperFeatureExtractor's numpy path, restated in
// include/tdvc.h). The encoder stands on tdvc_wavlm_gemm and tdvc_wavlm_layernorm (ssl_wavlm.hip); this file holds the rest:
//
// tdvc_whisper_log_mel     two launches: a block per 8 frames (dft400.h, float64) writes log10(max(mel, 1e-10)) and its block maximum
//                          into the workspace, then a block per 8 frames takes the row maximum and stores max(., rowmax - 8) / 4 + 1
// tdvc_whisper_attention   the attention tile of attn_tile.h without gate and bias table
// tdvc_whisper_embed       x[b] = embed_tokens[ids[b][p]] + embed_positions[p], p from the device counter
// tdvc_whisper_linear_step the skinny GEMM of the decoder step, below
// tdvc_whisper_attn_step   one query per (row, head) against len keys, len = p + 1 from the device counter or a fixed count
// tdvc_whisper_logits      the final LayerNorm and the tied projection through the skinny GEMM, suppression, a (max, argmax) partial
//                          per workgroup
// tdvc_whisper_pick        the partials in a fixed order with lowest-index ties, forced prompt tokens, eos / pad, the counter
//
// The skinny GEMM: y[b][n] = epi(LN?(x[b]) . W[n] + bias[n]) for b < B <= 16 on v_mfma_f32_16x16x4_f32 (exact fp32). The MFMA's M index
// is the output column and its N index the batch row (rows at and past B are zeros), so a lane ends with four consecutive columns of
// one row. A workgroup of 512 threads (8 waves) owns 16 columns at a time (a few such tiles in turn where N is wide). Each weight is
// used once per step: a lane loads its float4 of W straight from global memory into registers; only the 16 input rows sit in LDS, in
// chunks of 1024 values per row. The reduction index of a chunk is split over the waves in pieces of 128; a wave sums its piece
// into two alternating accumulators, the waves' sums pass through LDS and wave 0 adds them in the order 0 .. 7. The LayerNorm
// prologue (K <= 1024: the whole row is one chunk) takes float64 statistics per row and rounds once, as tdvc_wavlm_layernorm does.
// A row's result depends on that row only: a row in a batch gets the bits it gets alone. No atomics, no host synchronisation.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "attn_tile.h"
#include "dft400.h"
#include "reduce.h"

namespace tdvc {

constexpr int WH_ROWS = 16;                                   // rows of a step launch: the MFMA's 16
constexpr int WH_MAXD = 1024;                                 // LayerNorm prologue, embed: d <= 1024
constexpr int LS_THREADS = 512, LS_WAVES = 8, LS_KC = 1024, LS_LD = LS_KC + 4, LS_PIECE = LS_KC / LS_WAVES;
constexpr int LS_MAX_TILES = 8;                               // column tiles of 16 a workgroup takes in turn
constexpr int AS_THREADS = 512, AS_WAVES = 8;
constexpr int MEL_MAX = 128;

typedef float wh_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wh_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// ---------------------------------------------------------------------------------------------------------------- log-mel
struct MelP {
  const float* x; long x_bs; const int* lengths;
  int L, n_samples, frames, n_mels, nblk;
  const double* table;
  double* logmel;           // [B][frames][n_mels]
  double* blkmax;           // [B][nblk]
  float* y; long y_bs, y_ms, y_fs;
};

__global__ __launch_bounds__(256) void whisper_mel_kernel(MelP p) {
  __shared__ __attribute__((aligned(16))) double cs[2 * DFT_NFFT];
  __shared__ __attribute__((aligned(16))) double xw[DFT_FR][DFT_NFFT];
  __shared__ __attribute__((aligned(16))) double pw[DFT_FR][DFT_BINS];
  __shared__ double red[4];
  const int t = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * DFT_FR;
  const int len = min(row_len(p.lengths, b, p.L), p.n_samples);           // samples at and past len are zeros and are never read
  const float* xr = p.x + b * p.x_bs;
  for (int i = t; i < 2 * DFT_NFFT; i += 256) cs[i] = p.table[i];
  for (int item = t; item < DFT_FR * DFT_NFFT; item += 256) {
    const int fr = item / DFT_NFFT, i = item - fr * DFT_NFFT;
    int j = (f0 + fr) * DFT_HOP + i - DFT_NFFT / 2;                         // center=True: reflect padding of 200 around n_samples
    if (j < 0) j = -j;
    if (j >= p.n_samples) j = 2 * (p.n_samples - 1) - j;
    const double s = f0 + fr < p.frames && j >= 0 && j < len ? (double)xr[j] : 0.0;
    xw[fr][i] = s * p.table[DFT_TAB_WINDOW + i];
  }
  __syncthreads();
  dft400_power<256>(cs, xw, pw, t);
  __syncthreads();
  double mx = -INFINITY;
  for (int item = t; item < DFT_FR * p.n_mels; item += 256) {
    const int fr = item / p.n_mels, m = item - fr * p.n_mels;
    if (f0 + fr >= p.frames) continue;
    const double* fb = p.table + DFT_TAB_FB + (long)m * DFT_BINS;
    double a = 0.0;
    for (int k = 0; k < DFT_BINS; ++k) a = fma(fb[k], pw[fr][k], a);
    const double v = log10(fmax(a, 1e-10));
    p.logmel[((long)b * p.frames + f0 + fr) * p.n_mels + m] = v;
    mx = fmax(mx, v);
  }
  mx = block_max<4>(mx, red, t);
  if (t == 0) p.blkmax[(long)b * p.nblk + blockIdx.x] = mx;
}

__global__ __launch_bounds__(256) void whisper_mel_norm_kernel(MelP p) {
  __shared__ double red[4];
  const int t = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * DFT_FR;
  double mx = -INFINITY;
  for (int i = t; i < p.nblk; i += 256) mx = fmax(mx, p.blkmax[(long)b * p.nblk + i]);
  mx = block_max<4>(mx, red, t);
  for (int item = t; item < DFT_FR * p.n_mels; item += 256) {
    const int fr = item / p.n_mels, m = item - fr * p.n_mels;
    if (f0 + fr >= p.frames) continue;
    const double v = fmax(p.logmel[((long)b * p.frames + f0 + fr) * p.n_mels + m], mx - 8.0);
    p.y[b * p.y_bs + m * p.y_ms + (long)(f0 + fr) * p.y_fs] = (float)((v + 4.0) / 4.0);
  }
}

// ------------------------------------------------------------------------------------------------------------------ embed
__global__ __launch_bounds__(256) void whisper_embed_kernel(const int* ids, long ids_ld, const int* pos, int max_pos, const float* tok, const float* posw,
                                                            int d, int vocab, float* x, long x_bs) {
  const int b = blockIdx.x;
  const int p = min(max(*pos, 0), max_pos - 1);
  const int id = min(max(ids[b * ids_ld + p], 0), vocab - 1);
  for (int c = threadIdx.x; c < d; c += 256) x[b * x_bs + c] = tok[(long)id * d + c] + posw[(long)p * d + c];
}

// ------------------------------------------------------------------------------------------------------------- skinny GEMM
struct LinP {
  int B, N, K, tiles, gelu, scale_lo, scale_hi;
  float scale;
  const float* x; long x_bs;
  const float* gamma; const float* beta;
  const float* w; const float* bias;
  const float* res; long r_bs;
  float* y; long y_bs;
  // the cache epilogue: a column n >= cache_lo goes to kc (n - cache_lo < cache_d) or vc at position *pos
  int cache_lo, cache_d, cache_len; const int* pos; float* kc; float* vc; long c_bs;
  // the logits epilogue: raw values to y (may be null), suppression, a (max, argmax) partial per workgroup and row
  int logits, n_prompt; const unsigned char* mask; float* pmax; int* parg; int nwg;
};

__global__ __launch_bounds__(LS_THREADS) void whisper_linear_kernel(LinP p) {
  __shared__ __attribute__((aligned(16))) float xs[WH_ROWS * LS_LD];
  __shared__ __attribute__((aligned(16))) float red[LS_WAVES * 256];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = lane & 15, q = lane >> 4;
  const int nchunks = (p.K + LS_KC - 1) / LS_KC;
  int pos = 0;
  if (p.pos) pos = *p.pos;
  float best = -INFINITY;
  int best_n = 0x7fffffff;

  auto stage = [&](int c0) {                                                // the chunk [c0, c0 + LS_KC) of every row; zeros past K and past B
    for (int u = t; u < WH_ROWS * (LS_KC / 4); u += LS_THREADS) {
      const int r = u / (LS_KC / 4), c = 4 * (u - r * (LS_KC / 4));
      float4 v = float4{0.f, 0.f, 0.f, 0.f};
      if (r < p.B && c0 + c < p.K) v = *reinterpret_cast<const float4*>(p.x + r * p.x_bs + c0 + c);
      *reinterpret_cast<float4*>(xs + r * LS_LD + c) = v;
    }
    __syncthreads();
    if (p.gamma) {                                                          // K <= LS_KC: the whole row. Wave w takes the rows w and w + 8
      for (int r = w; r < p.B; r += LS_WAVES) {
        float* xr = xs + r * LS_LD;                                         // the row is read three times from LDS, not held in registers
        double s = 0.0;
        for (int c = lane; c < p.K; c += 64) s += (double)xr[c];
        const double mean = wave_sum(s) / (double)p.K;
        double ss = 0.0;
        for (int c = lane; c < p.K; c += 64) {
          const double dlt = (double)xr[c] - mean;
          ss = fma(dlt, dlt, ss);
        }
        const double rstd = 1.0 / sqrt(wave_sum(ss) / (double)p.K + 1e-5);
        for (int c = lane; c < p.K; c += 64) xr[c] = (float)(((double)xr[c] - mean) * rstd * (double)p.gamma[c] + (double)p.beta[c]);
      }
      __syncthreads();
    }
  };

  for (int tile = 0; tile < p.tiles; ++tile) {
    const int n0 = (blockIdx.x * p.tiles + tile) * 16;                      // block-uniform
    if (n0 >= p.N) break;
    const float* wrow = n0 + j < p.N ? p.w + (long)(n0 + j) * p.K : nullptr;
    wh_f32x4 acc = wh_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunks; ++ch) {
      const int kb = ch * LS_KC + w * LS_PIECE;                             // this wave's piece of the chunk
      float4 wr[LS_PIECE / 16];                                             // issued first: in flight while the input rows are staged
#pragma unroll
      for (int h = 0; h < LS_PIECE / 16; ++h) {
        const int k = kb + 16 * h + 4 * q;
        wr[h] = wrow && k < p.K ? *reinterpret_cast<const float4*>(wrow + k) : float4{0.f, 0.f, 0.f, 0.f};
      }
      if (nchunks > 1) {
        if (ch || tile) __syncthreads();                                    // the previous chunk has been read
        stage(ch * LS_KC);
      } else if (tile == 0) {
        stage(0);
      }
      wh_f32x4 a0 = wh_f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
      for (int h = 0; h < LS_PIECE / 16; h += 2) {
        const float4 v0 = *reinterpret_cast<const float4*>(xs + j * LS_LD + w * LS_PIECE + 16 * h + 4 * q);
        const float4 v1 = *reinterpret_cast<const float4*>(xs + j * LS_LD + w * LS_PIECE + 16 * h + 16 + 4 * q);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h].x, v0.x, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h + 1].x, v1.x, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h].y, v0.y, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h + 1].y, v1.y, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h].z, v0.z, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h + 1].z, v1.z, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h].w, v0.w, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[h + 1].w, v1.w, a1, 0, 0, 0);
      }
      acc += a0 + a1;
    }
    if (tile) __syncthreads();                                              // red of the previous tile has been read
    *reinterpret_cast<wh_f32x4*>(red + w * 256 + lane * 4) = acc;
    __syncthreads();
    if (w == 0) {
      wh_f32x4 s = *reinterpret_cast<const wh_f32x4*>(red + lane * 4);
#pragma unroll
      for (int ww = 1; ww < LS_WAVES; ++ww) s += *reinterpret_cast<const wh_f32x4*>(red + ww * 256 + lane * 4);
      const int n = n0 + 4 * q;                                             // this lane: row j, the columns n .. n + 3
      if (j < p.B && n < p.N) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nn = min(n + r, p.N - 1);
          v[r] = (s[r] + (p.bias ? p.bias[nn] : 0.f)) * (nn >= p.scale_lo && nn < p.scale_hi ? p.scale : 1.f);
          if (p.gelu) v[r] = wh_gelu(v[r]);
        }
        if (p.logits) {
          for (int r = 0; r < 4 && n + r < p.N; ++r) {
            if (p.y) p.y[j * p.y_bs + n + r] = v[r];
            const unsigned char mk = p.mask ? p.mask[n + r] : 0;
            const float sv = (mk & 1) || ((mk & 2) && pos == p.n_prompt - 1) ? -INFINITY : v[r];
            if (sv > best || (sv == best && n + r < best_n)) { best = sv; best_n = n + r; }
          }
        } else {                                                            // N is a multiple of 16 here
          if (p.res) {
            const float4 rr = *reinterpret_cast<const float4*>(p.res + j * p.r_bs + n);
            v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
          }
          float* dst = p.y + j * p.y_bs + n;
          if (p.kc && n >= p.cache_lo) {
            const int c = n - p.cache_lo, at = min(max(pos, 0), p.cache_len - 1);
            dst = (c < p.cache_d ? p.kc + c : p.vc + (c - p.cache_d)) + j * p.c_bs + (long)at * p.cache_d;
          }
          *reinterpret_cast<float4*>(dst) = float4{v[0], v[1], v[2], v[3]};
        }
      }
    }
  }
  if (p.logits && w == 0) {                                                 // the four column groups of a row sit 16 lanes apart
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float ob = __shfl_xor(best, off);
      const int on = __shfl_xor(best_n, off);
      if (ob > best || (ob == best && on < best_n)) { best = ob; best_n = on; }
    }
    if (q == 0 && j < p.B) {
      p.pmax[(long)j * p.nwg + blockIdx.x] = best;
      p.parg[(long)j * p.nwg + blockIdx.x] = best_n;
    }
  }
}

// --------------------------------------------------------------------------------------------------------- attention step
struct AStepP {
  const float* q; long q_bs;
  const float* k; const float* v; long kv_bs, kv_ts;
  const int* pos; int len, max_len;
  float* out; long o_bs;
};

// A workgroup per (row, head), 8 waves; wave w takes the key tiles w, w + 8, .. of 64 keys. In a tile a lane scores one key (its row of
// K straight from global memory), the probabilities pass through LDS, then lane = (group g, float4 c4 of the head) adds p v over
// the keys g, g + G, .. of the tile. At the end the groups of a wave are added in the order 0 .. G - 1 and the waves in the order
// 0 .. 7 with the usual rescaling. Keys at and past len are never read.
template <int D>
__global__ __launch_bounds__(AS_THREADS) void whisper_attn_step_kernel(AStepP p) {
  constexpr int DQ = D / 4, G = 64 / DQ;
  __shared__ float ps[AS_WAVES][64];
  __shared__ __attribute__((aligned(16))) float part[AS_WAVES][G][D];
  __shared__ float wm[AS_WAVES], wl[AS_WAVES];
  __shared__ __attribute__((aligned(16))) float wacc[AS_WAVES][D];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.y, n = blockIdx.x;
  const int len = p.pos ? min(max(*p.pos, 0) + 1, p.max_len) : p.len;
  const float* qr = p.q + b * p.q_bs + n * D;
  const float* kb = p.k + b * p.kv_bs + n * D;
  const float* vb = p.v + b * p.kv_bs + n * D;
  float4 q4[DQ];
#pragma unroll
  for (int c = 0; c < DQ; ++c) q4[c] = *reinterpret_cast<const float4*>(qr + 4 * c);
  const int g = lane / DQ, c4 = lane - g * DQ;
  float m = -INFINITY, l = 0.f;
  float4 acc = float4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = w * 64; s0 < len; s0 += AS_WAVES * 64) {
    const int s = s0 + lane;
    float a = -INFINITY;
    if (s < len) {
      const float* kr = kb + (long)s * p.kv_ts;
      a = 0.f;
#pragma unroll
      for (int c = 0; c < DQ; ++c) {
        const float4 k4 = *reinterpret_cast<const float4*>(kr + 4 * c);
        a = fmaf(q4[c].x, k4.x, a); a = fmaf(q4[c].y, k4.y, a); a = fmaf(q4[c].z, k4.z, a); a = fmaf(q4[c].w, k4.w, a);
      }
    }
    const float mn = fmaxf(m, wave_max(a));                                 // finite: the tile holds a key below len
    const float alpha = expf(m - mn);                                       // 0 in the wave's first tile
    const float pe = s < len ? expf(a - mn) : 0.f;
    ps[w][lane] = pe;
    l = fmaf(l, alpha, wave_sum(pe));
    m = mn;
    acc.x *= alpha; acc.y *= alpha; acc.z *= alpha; acc.w *= alpha;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // every load of the tile is issued before the first use (a loop with a run-time bound waits for each load in turn). A key at or
    // past len has p = 0 and reads the row of the last key below len instead.
    const int last = len - 1 - s0;
    float4 vr[64 / G];
#pragma unroll
    for (int i = 0; i < 64 / G; ++i) vr[i] = *reinterpret_cast<const float4*>(vb + (long)(s0 + min(g + G * i, last)) * p.kv_ts + 4 * c4);
#pragma unroll
    for (int i = 0; i < 64 / G; ++i) {
      const float pv = ps[w][g + G * i];
      acc.x = fmaf(pv, vr[i].x, acc.x); acc.y = fmaf(pv, vr[i].y, acc.y); acc.z = fmaf(pv, vr[i].z, acc.z); acc.w = fmaf(pv, vr[i].w, acc.w);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  *reinterpret_cast<float4*>(&part[w][g][4 * c4]) = acc;
  if (lane == 0) { wm[w] = m; wl[w] = l; }
  __syncthreads();
  if (lane < D) {
    float s = part[w][0][lane];
#pragma unroll
    for (int gg = 1; gg < G; ++gg) s += part[w][gg][lane];
    wacc[w][lane] = s;
  }
  __syncthreads();
  if (t < D) {
    float mm = wm[0];
#pragma unroll
    for (int ww = 1; ww < AS_WAVES; ++ww) mm = fmaxf(mm, wm[ww]);
    float ll = 0.f, o = 0.f;
#pragma unroll
    for (int ww = 0; ww < AS_WAVES; ++ww) {
      const float sc = wm[ww] == -INFINITY ? 0.f : expf(wm[ww] - mm);      // a wave without keys
      ll = fmaf(wl[ww], sc, ll);
      o = fmaf(wacc[ww][t], sc, o);
    }
    p.out[b * p.o_bs + n * D + t] = o / ll;
  }
}

// ------------------------------------------------------------------------------------------------------------------- pick
struct PickP {
  int B, nwg, n_prompt, total, eos, pad;
  const float* pmax; const int* parg;
  int* ids; long ids_ld; int* pos; int* n_tokens; int* finished; int* all_done;
};

// one workgroup: the rows in turn, then the counter. Every thread reads the counter before the first barrier; thread 0 writes it last.
__global__ __launch_bounds__(256) void whisper_pick_kernel(PickP p) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int t = threadIdx.x, pos = *p.pos;
  if (pos < 0 || pos + 1 >= p.total) return;                                // block-uniform: no slot for another token
  int done = 1;
  for (int b = 0; b < p.B; ++b) {
    float best = -INFINITY;
    int best_n = 0x7fffffff;
    for (int i = t; i < p.nwg; i += 256) {
      const float v = p.pmax[(long)b * p.nwg + i];
      const int n = p.parg[(long)b * p.nwg + i];
      if (v > best || (v == best && n < best_n)) { best = v; best_n = n; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int on = __shfl_xor(best_n, off);
      if (ob > best || (ob == best && on < best_n)) { best = ob; best_n = on; }
    }
    __syncthreads();                                                        // bv, bi of the previous row have been read
    if ((t & 63) == 0) { bv[t >> 6] = best; bi[t >> 6] = best_n; }
    __syncthreads();
    if (t == 0) {
      for (int ww = 1; ww < 4; ++ww)
        if (bv[ww] > best || (bv[ww] == best && bi[ww] < best_n)) { best = bv[ww]; best_n = bi[ww]; }
      if (pos + 1 >= p.n_prompt) {                                          // a prompt token is already in its place
        int tok = p.pad;
        if (!p.finished[b]) {
          tok = best_n;
          p.n_tokens[b] = pos + 2;
          if (tok == p.eos) p.finished[b] = 1;
        }
        p.ids[b * p.ids_ld + pos + 1] = tok;
      } else {
        p.n_tokens[b] = pos + 2;
      }
      done &= p.finished[b] != 0;
    }
  }
  if (t == 0) {
    *p.all_done = done;
    *p.pos = pos + 1;
  }
}

static bool misaligned(const void* a) { return ((uintptr_t)a & 15) != 0; }

static int lin_tiles(int N) {                                               // about 1024 workgroups where N is wide
  const int nt = (N + 15) / 16;
  int tiles = nt / 1024;
  if (tiles < 1) tiles = 1;
  if (tiles > LS_MAX_TILES) tiles = LS_MAX_TILES;
  return tiles;
}

}  // namespace tdvc

using namespace tdvc;

extern "C" size_t tdvc_whisper_log_mel_workspace(int32_t B, int32_t n_samples, int32_t n_mels) {
  if (B < 0 || n_samples < DFT_HOP || n_mels < 1) return 0;
  const size_t frames = (size_t)n_samples / DFT_HOP, nblk = (frames + DFT_FR - 1) / DFT_FR;
  return tdvc_align256((size_t)B * frames * n_mels * sizeof(double)) + tdvc_align256((size_t)B * nblk * sizeof(double));
}

extern "C" int tdvc_whisper_log_mel(const float* x, int64_t x_bs, const int32_t* lengths, int32_t B, int32_t L, int32_t n_samples, const double* table,
                                    int32_t n_mels, float* y, int64_t y_bs, int64_t y_ms, int64_t y_fs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (B < 0 || L < 0 || n_samples < 0 || x_bs < 0 || y_bs < 0 || y_ms < 0 || y_fs < 0) return tdvc_fail(TDVC_EINVAL, "whisper_log_mel: negative size or stride");
  if (n_mels < 1 || n_mels > MEL_MAX) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_log_mel: 1 to 128 mel bands");
  if (n_samples % DFT_HOP || n_samples < DFT_NFFT) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_log_mel: n_samples must be a multiple of the hop 160 and at least 400");
  if (n_samples > (1 << 28) || L > (1 << 30) || B > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_log_mel: n_samples > 2^28, L > 2^30 or B > 65535");
  if (B == 0) return TDVC_OK;
  if (!x || !table || !y || !workspace) return tdvc_fail(TDVC_EINVAL, "whisper_log_mel: null pointer");
  if (workspace_bytes < tdvc_whisper_log_mel_workspace(B, n_samples, n_mels)) return tdvc_fail(TDVC_EINVAL, "whisper_log_mel: workspace too small");
  MelP p;
  p.x = x; p.x_bs = x_bs; p.lengths = lengths; p.L = L; p.n_samples = n_samples; p.frames = n_samples / DFT_HOP; p.n_mels = n_mels;
  p.nblk = (p.frames + DFT_FR - 1) / DFT_FR; p.table = table;
  p.logmel = (double*)workspace;
  p.blkmax = (double*)((char*)workspace + tdvc_align256((size_t)B * p.frames * n_mels * sizeof(double)));
  p.y = y; p.y_bs = y_bs; p.y_ms = y_ms; p.y_fs = y_fs;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(whisper_mel_kernel, dim3(p.nblk, B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(whisper_mel_norm_kernel, dim3(p.nblk, B), dim3(256), 0, st, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_whisper_attention(const float* q, const float* k, const float* v, int64_t bs, int64_t ts, int32_t B, int32_t T, int32_t H, int32_t d,
                                      float* out, int64_t o_bs, int64_t o_ts, void* stream) {
  if (B < 0 || T < 0 || H < 1 || d < 1 || bs < 0 || ts < 0 || o_bs < 0 || o_ts < 0) return tdvc_fail(TDVC_EINVAL, "whisper_attention: negative size or stride");
  if (d != 16 && d != 32 && d != 64) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_attention: the head width must be 16, 32 or 64");
  if (T > AT_MAXT) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_attention: more than 4096 tokens");
  if (B > 65535 || H > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_attention: B or H > 65535");
  if ((bs | ts | o_bs | o_ts) & 3) return tdvc_fail(TDVC_EINVAL, "whisper_attention: strides must be multiples of 4 floats");
  if (ts < (int64_t)H * d || o_ts < (int64_t)H * d) return tdvc_fail(TDVC_EINVAL, "whisper_attention: token stride below H d");
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(out)) return tdvc_fail(TDVC_EINVAL, "whisper_attention: q, k, v and out must be 16-byte aligned");
  if (B == 0 || T == 0) return TDVC_OK;
  if (!q || !k || !v || !out) return tdvc_fail(TDVC_EINVAL, "whisper_attention: null pointer");
  AttnP p;
  p.q = q; p.k = k; p.v = v; p.bs = bs; p.ts = ts; p.T = T; p.H = H; p.gate = nullptr; p.bias_rel = nullptr; p.out = out; p.o_bs = o_bs; p.o_ts = o_ts;
  attn_tile_launch<false>(p, B, d, (hipStream_t)stream);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_whisper_embed(const int32_t* ids, int64_t ids_ld, const int32_t* pos, int32_t max_pos, const float* embed_tokens,
                                  const float* embed_positions, int32_t B, int32_t d, int32_t vocab, float* x, int64_t x_bs, void* stream) {
  if (B < 0 || d < 1 || vocab < 1 || max_pos < 1 || ids_ld < 0 || x_bs < 0) return tdvc_fail(TDVC_EINVAL, "whisper_embed: negative size or stride");
  if (B > WH_ROWS) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_embed: more than 16 rows in a step launch");
  if (d % 16 || d > WH_MAXD) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_embed: d must be a multiple of 16 up to 1024");
  if (ids_ld < max_pos || x_bs < d) return tdvc_fail(TDVC_EINVAL, "whisper_embed: a row of ids holds max_pos tokens, a row of x d values");
  if (B == 0) return TDVC_OK;
  if (!ids || !pos || !embed_tokens || !embed_positions || !x) return tdvc_fail(TDVC_EINVAL, "whisper_embed: null pointer");
  hipLaunchKernelGGL(whisper_embed_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ids, (long)ids_ld, pos, max_pos, embed_tokens, embed_positions, d, vocab,
                     x, (long)x_bs);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_whisper_linear_step(const tdvc_whisper_linear_args* a, void* stream) {
  if (!a) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: null arguments");
  if (a->B < 0 || a->N < 1 || a->K < 1 || a->x_bs < 0 || a->r_bs < 0 || a->y_bs < 0 || a->c_bs < 0 || a->cache_len < 0 || a->cache_lo < 0)
    return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: negative size or stride");
  if (a->B > WH_ROWS) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_linear_step: more than 16 rows in a step launch");
  if (a->N % 16 || a->K % 16) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_linear_step: N and K must be multiples of 16");
  if (a->N > (1 << 24) || a->K > (1 << 20)) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_linear_step: N > 2^24 or K > 2^20");
  if (a->epilogue < 0 || a->epilogue > 1) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: epilogue must be 0 (none) or 1 (erf-GELU)");
  if ((a->gamma != nullptr) != (a->beta != nullptr)) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: the LayerNorm prologue needs gamma and beta");
  if (a->gamma && a->K > WH_MAXD) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_linear_step: the LayerNorm prologue takes rows of up to 1024");
  if ((a->x_bs | a->r_bs | a->y_bs | a->c_bs) & 3) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: strides must be multiples of 4 floats");
  if (a->x_bs < a->K) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: input row stride below K");
  if (misaligned(a->x) || misaligned(a->w) || misaligned(a->res) || misaligned(a->y) || misaligned(a->k_cache) || misaligned(a->v_cache))
    return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: x, w, residual, y and the caches must be 16-byte aligned");
  const bool cache = a->k_cache || a->v_cache;
  int cache_d = 0;
  if (cache) {
    if (!a->k_cache || !a->v_cache || !a->pos) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: the cache epilogue needs k_cache, v_cache and the position counter");
    if (a->cache_lo % 16 || a->cache_lo > a->N || (a->N - a->cache_lo) % 32 || a->cache_lo == a->N)
      return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: the columns from cache_lo are k | v of equal widths, multiples of 16");
    cache_d = (a->N - a->cache_lo) / 2;
    if (a->cache_len < 1 || a->c_bs < (int64_t)a->cache_len * cache_d) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: a cache row holds cache_len positions");
    if (a->res) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: no residual with the cache epilogue");
  }
  const int ny = cache ? a->cache_lo : a->N;                                // columns that go to y
  if (ny > 0 && a->y_bs < ny) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: output row stride below the columns written");
  if (a->res && a->r_bs < a->N) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: residual row stride below N");
  if (a->B == 0) return TDVC_OK;
  if (!a->x || !a->w || (ny > 0 && !a->y)) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: null pointer");
  if (a->y == a->x) return tdvc_fail(TDVC_EINVAL, "whisper_linear_step: y must not be x (every workgroup reads whole rows of x)");
  LinP p = {};
  p.B = a->B; p.N = a->N; p.K = a->K; p.tiles = lin_tiles(a->N); p.gelu = a->epilogue; p.scale_lo = a->scale_lo; p.scale_hi = a->scale_hi; p.scale = a->scale;
  p.x = a->x; p.x_bs = a->x_bs; p.gamma = a->gamma; p.beta = a->beta; p.w = a->w; p.bias = a->bias; p.res = a->res; p.r_bs = a->r_bs; p.y = a->y; p.y_bs = a->y_bs;
  p.cache_lo = a->cache_lo; p.cache_d = cache_d; p.cache_len = a->cache_len; p.pos = cache ? a->pos : nullptr; p.kc = a->k_cache; p.vc = a->v_cache; p.c_bs = a->c_bs;
  const int nt = a->N / 16, grid = (nt + p.tiles - 1) / p.tiles;
  hipLaunchKernelGGL(whisper_linear_kernel, dim3(grid), dim3(LS_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_whisper_attn_step(const float* q, int64_t q_bs, const float* k, const float* v, int64_t kv_bs, int64_t kv_ts, const int32_t* pos,
                                      int32_t len, int32_t B, int32_t H, int32_t d, float* out, int64_t o_bs, void* stream) {
  if (B < 0 || H < 1 || d < 1 || len < 1 || q_bs < 0 || kv_bs < 0 || kv_ts < 0 || o_bs < 0) return tdvc_fail(TDVC_EINVAL, "whisper_attn_step: negative size or stride, or no key");
  if (B > WH_ROWS) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_attn_step: more than 16 rows in a step launch");
  if (d != 16 && d != 32 && d != 64) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_attn_step: the head width must be 16, 32 or 64");
  if (len > AT_MAXT || H > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_attn_step: more than 4096 keys or H > 65535");
  if ((q_bs | kv_bs | kv_ts | o_bs) & 3) return tdvc_fail(TDVC_EINVAL, "whisper_attn_step: strides must be multiples of 4 floats");
  if (kv_ts < (int64_t)H * d || q_bs < (int64_t)H * d || o_bs < (int64_t)H * d || kv_bs < (int64_t)len * kv_ts)
    return tdvc_fail(TDVC_EINVAL, "whisper_attn_step: a stride below H d, or a key row shorter than len positions");
  if (misaligned(q) || misaligned(k) || misaligned(v) || misaligned(out)) return tdvc_fail(TDVC_EINVAL, "whisper_attn_step: q, k, v and out must be 16-byte aligned");
  if (B == 0) return TDVC_OK;
  if (!q || !k || !v || !out) return tdvc_fail(TDVC_EINVAL, "whisper_attn_step: null pointer");
  AStepP p;
  p.q = q; p.q_bs = q_bs; p.k = k; p.v = v; p.kv_bs = kv_bs; p.kv_ts = kv_ts; p.pos = pos; p.len = len; p.max_len = len; p.out = out; p.o_bs = o_bs;
  const dim3 grid(H, B);
  hipStream_t st = (hipStream_t)stream;
  if (d == 16) hipLaunchKernelGGL(whisper_attn_step_kernel<16>, grid, dim3(AS_THREADS), 0, st, p);
  else if (d == 32) hipLaunchKernelGGL(whisper_attn_step_kernel<32>, grid, dim3(AS_THREADS), 0, st, p);
  else hipLaunchKernelGGL(whisper_attn_step_kernel<64>, grid, dim3(AS_THREADS), 0, st, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" size_t tdvc_whisper_workspace(int32_t d, int32_t decoder_layers, int32_t vocab, int32_t B, int32_t T_enc, int32_t max_len, int64_t* offsets) {
  if (d < 1 || decoder_layers < 1 || vocab < 1 || B < 0 || T_enc < 0 || max_len < 0) return 0;
  const int nt = (vocab + 15) / 16, tiles = lin_tiles(vocab), nwg = (nt + tiles - 1) / tiles;
  const size_t self_kv = tdvc_align256((size_t)2 * decoder_layers * B * max_len * d * sizeof(float));
  const size_t cross_kv = tdvc_align256((size_t)2 * decoder_layers * B * T_enc * d * sizeof(float));
  const size_t partials = tdvc_align256((size_t)WH_ROWS * nwg * (sizeof(float) + sizeof(int32_t)));
  if (offsets) { offsets[0] = 0; offsets[1] = (int64_t)self_kv; offsets[2] = (int64_t)(self_kv + cross_kv); offsets[3] = nwg; }
  return self_kv + cross_kv + partials;
}

extern "C" int tdvc_whisper_logits(const float* x, int64_t x_bs, const float* gamma, const float* beta, const float* embed_tokens, int32_t B, int32_t d,
                                   int32_t vocab, const uint8_t* mask, const int32_t* pos, int32_t n_prompt, float* logits, int64_t l_bs, void* partials,
                                   size_t partial_bytes, void* stream) {
  if (B < 0 || d < 1 || vocab < 1 || x_bs < 0 || l_bs < 0 || n_prompt < 1) return tdvc_fail(TDVC_EINVAL, "whisper_logits: negative size or stride, or an empty prompt");
  if (B > WH_ROWS) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_logits: more than 16 rows in a step launch");
  if (d % 16 || d > WH_MAXD) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_logits: d must be a multiple of 16 up to 1024");
  if (vocab > (1 << 24)) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_logits: vocab > 2^24");
  if (x_bs & 3 || x_bs < d) return tdvc_fail(TDVC_EINVAL, "whisper_logits: the row stride of x must be a multiple of 4 floats, at least d");
  if (logits && l_bs < vocab) return tdvc_fail(TDVC_EINVAL, "whisper_logits: logits row stride below vocab");
  if (misaligned(x) || misaligned(embed_tokens)) return tdvc_fail(TDVC_EINVAL, "whisper_logits: x and embed_tokens must be 16-byte aligned");
  const int nt = (vocab + 15) / 16, tiles = lin_tiles(vocab), nwg = (nt + tiles - 1) / tiles;
  if (B == 0) return TDVC_OK;
  if (!x || !gamma || !beta || !embed_tokens || !pos || !partials) return tdvc_fail(TDVC_EINVAL, "whisper_logits: null pointer");
  if (partial_bytes < (size_t)WH_ROWS * nwg * (sizeof(float) + sizeof(int32_t))) return tdvc_fail(TDVC_EINVAL, "whisper_logits: workspace too small");
  LinP p = {};
  p.B = B; p.N = vocab; p.K = d; p.tiles = tiles; p.scale = 1.f; p.x = x; p.x_bs = x_bs; p.gamma = gamma; p.beta = beta; p.w = embed_tokens;
  p.y = logits; p.y_bs = l_bs; p.pos = pos; p.logits = 1; p.n_prompt = n_prompt; p.mask = mask;
  p.pmax = (float*)partials; p.parg = (int*)((float*)partials + (size_t)WH_ROWS * nwg); p.nwg = nwg;
  hipLaunchKernelGGL(whisper_linear_kernel, dim3(nwg), dim3(LS_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_whisper_pick(const void* partials, size_t partial_bytes, int32_t vocab, int32_t B, int32_t* ids, int64_t ids_ld, int32_t n_prompt,
                                 int32_t total, int32_t eos, int32_t pad, int32_t* pos, int32_t* n_tokens, int32_t* finished, int32_t* all_done, void* stream) {
  if (B < 0 || vocab < 1 || ids_ld < 0 || n_prompt < 1 || total < n_prompt) return tdvc_fail(TDVC_EINVAL, "whisper_pick: negative size, an empty prompt or total below the prompt");
  if (B > WH_ROWS) return tdvc_fail(TDVC_EUNSUPPORTED, "whisper_pick: more than 16 rows in a step launch");
  if (ids_ld < total) return tdvc_fail(TDVC_EINVAL, "whisper_pick: a row of ids holds total tokens");
  if (eos < 0 || eos >= vocab || pad < 0 || pad >= vocab) return tdvc_fail(TDVC_EINVAL, "whisper_pick: eos and pad must be tokens of the vocabulary");
  const int nt = (vocab + 15) / 16, tiles = lin_tiles(vocab), nwg = (nt + tiles - 1) / tiles;
  if (B == 0) return TDVC_OK;
  if (!partials || !ids || !pos || !n_tokens || !finished || !all_done) return tdvc_fail(TDVC_EINVAL, "whisper_pick: null pointer");
  if (partial_bytes < (size_t)WH_ROWS * nwg * (sizeof(float) + sizeof(int32_t))) return tdvc_fail(TDVC_EINVAL, "whisper_pick: workspace too small");
  PickP p;
  p.B = B; p.nwg = nwg; p.n_prompt = n_prompt; p.total = total; p.eos = eos; p.pad = pad;
  p.pmax = (const float*)partials; p.parg = (const int*)((const float*)partials + (size_t)WH_ROWS * nwg);
  p.ids = ids; p.ids_ld = ids_ld; p.pos = pos; p.n_tokens = n_tokens; p.finished = finished; p.all_done = all_done;
  hipLaunchKernelGGL(whisper_pick_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
