// Sample-rate conversion and segment preparation of the data pipeline (data/dataset.py load_audio: resampy.resample with its
// defaults, util.eq_rms, gain / sign augmentation, crop, pad, additive noise) on the device.
//
// tdvc_resample: resampy's table-interpolated windowed sinc as a polyphase FIR. With sr_new / sr_orig reduced to L / M, output t
// sits at input n = (t*M) div L with phase (t*M) mod L, and its interpolated weights depend on the phase only, so the host
// (resample.py, numpy float64) tabulates them once per rate pair: W taps per phase, `left` of them at or before n, and
//     y[t] = sum_j w[phase(t)][j] * x[n - left + 1 + j],   x = 0 outside [0, n_in[b])
// which reproduces both of resampy's loop truncations. The table is indexed by the output's residue q = t mod L (column q holds
// phase (q*M) mod L) with caller-given strides, bank[j*ts + q*cs]. The product stores it tap-major, ts = L and cs = 1, so that the
// 64 lanes of a wave (consecutive t) read 64 consecutive doubles for every tap: one coalesced 512-byte load instead of a gather
// over 64 phase rows (ts = 1, cs = W, which tools/bench_resample.py times beside it). For L == 1 the address is wave-uniform and
// the weights come through the scalar cache.
// One 256-thread block per (row, tile of RS_TO = 256 outputs), one output per thread. The tile's input span, (RS_TO-1)*M/L + W
// samples, is staged in LDS as float64 (zero-extended there, so the inner loop has no bounds test and converts nothing); lane
// strides in LDS are M/L doubles: conflict-free at M = 3, L = 1, 2-way at worst where the stride alternates. The sum runs over
// the taps in ascending order in four interleaved float64 chains that are added at the end: a fixed order, no atomics, two calls
// give the same bits. The result is
// rounded once to fp32. Every element of y[b][0 .. n_out_max) is written, zeros past n_out[b]. x is never read at or past
// min(n_in[b], T). Each block also leaves the float64 sum of squares of its unrounded outputs in the workspace
// (tile_sq[b][tile]) for tdvc_segment's RMS.
//
// tdvc_segment: one 256-thread block per row. gain = 10^(db/20) / sqrt(sum / n) from the tile sums (or, with no tile sums, from
// the row itself), both reduced in a fixed order; then out[s] = x[start + s] * gain * aug_gain * aug_sign for s inside the crop
// and 0 behind it, + noise[s] * noise_scale, in float64 from the fp32 input and rounded once. Writes all of [B][S].
#include "../../include/tdvc.h"
#include "api_util.h"

namespace tdvc {

constexpr int RS_TO = 256;                                 // outputs per block (tdvc_resample_tile)
constexpr int RS_SPAN_MAX = 7680;                          // float64 input samples staged per tile: 60 KiB + 2 KiB reduction
constexpr size_t RS_BANK_MAX = (size_t)8 << 20;            // bytes
constexpr int SEG_THREADS = 256;

struct ResampleP {
  const float* x; long x_bs;
  const int* n_in; const int* n_out;
  const double* bank; long ts, cs;                         // weight of tap j for output residue q = t mod L: bank[j*ts + q*cs]
  int T, L, M, W, left, n_out_max, ntiles;
  float* y; long y_bs;
  double* tile_sq;                                         // [B][ntiles]
};

// fixed binary tree over the block's 256 values; the result is in red[0] after the call
__device__ __forceinline__ void block_sum_256(double* red, int tid) {
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
}

template <bool L1>
__global__ __launch_bounds__(RS_TO) void resample_kernel(ResampleP p) {
  extern __shared__ double rs_lds[];
  double* red = rs_lds;                                    // [RS_TO]
  double* xs = rs_lds + RS_TO;                             // [span]
  const int tid = threadIdx.x;
  const long b = blockIdx.y;
  const int tile = blockIdx.x;
  const int t0 = tile * RS_TO;
  const int n_in = min(p.n_in[b], p.T);
  const int n_out = min(p.n_out[b], p.n_out_max);
  const int cnt = min(RS_TO, p.n_out_max - t0);            // >= 1 by the grid
  const long nf = ((long)t0 * p.M) / p.L;                  // input position of the tile's first and last output
  const long nl = ((long)(t0 + cnt - 1) * p.M) / p.L;
  const int span = (int)(nl - nf) + p.W;                   // <= RS_SPAN_MAX (checked on the host)
  const bool live = t0 < n_out;                            // block-uniform: a tile past the row's end only writes zeros
  if (live) {
    const float* xr = p.x + b * p.x_bs;
    const long g0 = nf - p.left + 1;
    for (int i = tid; i < span; i += RS_TO) {
      const long g = g0 + i;
      xs[i] = (g >= 0 && g < n_in) ? (double)xr[g] : 0.0;
    }
  }
  __syncthreads();
  const int t = t0 + tid;
  double acc = 0.0;
  if (live && t < n_out) {
    const long tm = (long)t * p.M;
    const int q = L1 ? 0 : t % p.L;
    const double* __restrict__ w = p.bank + q * p.cs;
    const double* __restrict__ xp = xs + (int)(tm / p.L - nf);
    const long Ls = p.ts;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = 0;
    for (; j + 4 <= p.W; j += 4) {
      a0 = fma(w[(j + 0) * Ls], xp[j + 0], a0);
      a1 = fma(w[(j + 1) * Ls], xp[j + 1], a1);
      a2 = fma(w[(j + 2) * Ls], xp[j + 2], a2);
      a3 = fma(w[(j + 3) * Ls], xp[j + 3], a3);
    }
    for (; j < p.W; ++j) a0 = fma(w[j * Ls], xp[j], a0);
    acc = (a0 + a1) + (a2 + a3);
  }
  if (t < p.n_out_max) p.y[b * p.y_bs + t] = (float)acc;
  red[tid] = acc * acc;
  block_sum_256(red, tid);
  if (tid == 0) p.tile_sq[b * p.ntiles + tile] = red[0];
}

struct SegmentP {
  const float* x; long x_bs;
  const int* n;
  int T;                                                   // readable samples per row: n[b] is clamped to it
  const double* tile_sq; int ntiles;
  const int* start; const float* aug_gain; const float* aug_sign;
  const float* noise; long noise_bs; double noise_scale;
  double target;                                           // 10^(db/20); <= 0: no normalisation
  int max_segment, S;
  float* y;                                                // [B][S] dense
  double* gain;                                            // [B]
};

__global__ __launch_bounds__(SEG_THREADS) void segment_kernel(SegmentP p) {
  __shared__ double red[SEG_THREADS];
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const int n = max(0, min(p.n[b], p.T));
  const float* xr = p.x + b * p.x_bs;
  double g = 1.0;
  if (p.target > 0.0) {
    double s = 0.0;
    if (p.tile_sq) {
      const int used = (n + RS_TO - 1) / RS_TO;            // tiles past the row's end hold zeros: skipping them changes nothing
      for (int i = tid; i < min(used, p.ntiles); i += SEG_THREADS) s += p.tile_sq[b * p.ntiles + i];
    } else {
      for (int i = tid; i < n; i += SEG_THREADS) { const double v = (double)xr[i]; s = fma(v, v, s); }
    }
    red[tid] = s;
    block_sum_256(red, tid);
    const double ms = n > 0 ? red[0] / (double)n : 0.0;
    g = ms > 0.0 ? p.target / sqrt(ms) : 0.0;              // a silent row stays silent (the reference divides by zero here)
  }
  if (tid == 0 && p.gain) p.gain[b] = g;
  const bool crop = p.max_segment > 0 && n > p.max_segment;
  const int len = crop ? p.max_segment : n;
  int st = 0;
  if (crop && p.start) st = max(0, min(p.start[b], n - p.max_segment));
  const double ag = p.aug_gain ? (double)p.aug_gain[b] : 1.0;
  const double sg = p.aug_sign ? (p.aug_sign[b] < 0.f ? -1.0 : 1.0) : 1.0;
  const float* nr = p.noise ? p.noise + b * p.noise_bs : nullptr;
  float* yr = p.y + b * (long)p.S;
  for (int s = tid; s < p.S; s += SEG_THREADS) {
    double v = 0.0;
    if (s < len) v = ((double)xr[st + s] * g) * ag * sg;
    if (nr) v += (double)nr[s] * p.noise_scale;
    yr[s] = (float)v;
  }
}

static inline int rs_tiles(int n_out_max) { return (n_out_max + RS_TO - 1) / RS_TO; }

}  // namespace tdvc

extern "C" int32_t tdvc_resample_tile(void) { return tdvc::RS_TO; }

extern "C" size_t tdvc_resample_workspace(int32_t B, int32_t n_out_max) {
  if (B <= 0 || n_out_max <= 0) return 0;
  return (size_t)B * (size_t)tdvc::rs_tiles(n_out_max) * sizeof(double);
}

extern "C" int tdvc_resample(const float* x, int64_t x_bs, const int32_t* n_in, const int32_t* n_out, int32_t B, int32_t T, int32_t n_out_max,
                             const double* bank, int64_t bank_tap_stride, int64_t bank_col_stride, int32_t L, int32_t M, int32_t W,
                             int32_t left, float* y, int64_t y_bs,
                             void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || n_out_max < 0) return tdvc_fail(TDVC_EINVAL, "resample: negative size");
  if (L < 1 || M < 1 || W < 1 || left < 0 || left > W || bank_tap_stride < 1 || bank_col_stride < 1)
    return tdvc_fail(TDVC_EINVAL, "resample: bad polyphase bank geometry");
  if ((size_t)L * (size_t)W * sizeof(double) > RS_BANK_MAX)
    return tdvc_fail(TDVC_EUNSUPPORTED, "resample: the polyphase bank of this rate pair exceeds 8 MiB");
  const long span = ((long)(RS_TO - 1) * M) / L + 1 + W;
  if (span > RS_SPAN_MAX) return tdvc_fail(TDVC_EUNSUPPORTED, "resample: the input span of one output tile does not fit the LDS (ratio too small)");
  if (B == 0 || n_out_max == 0) return TDVC_OK;
  if (B > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "resample: more than 65535 rows");
  if (!x || !n_in || !n_out || !bank || !y) return tdvc_fail(TDVC_EINVAL, "resample: null pointer");
  if (x_bs < 0 || y_bs < n_out_max) return tdvc_fail(TDVC_EINVAL, "resample: bad row stride (output rows must not overlap)");
  if ((long)n_out_max * M / L + W > 0x7fffffffL) return tdvc_fail(TDVC_EUNSUPPORTED, "resample: row too long");
  const size_t need = tdvc_resample_workspace(B, n_out_max);
  if (!workspace || workspace_bytes < need) return tdvc_fail(TDVC_EWORKSPACE, "resample: workspace missing or too small");
  ResampleP p;
  p.x = x; p.x_bs = x_bs; p.n_in = n_in; p.n_out = n_out; p.bank = bank; p.ts = bank_tap_stride; p.cs = bank_col_stride;
  p.T = T; p.L = L; p.M = M; p.W = W; p.left = left; p.n_out_max = n_out_max; p.ntiles = rs_tiles(n_out_max);
  p.y = y; p.y_bs = y_bs; p.tile_sq = (double*)workspace;
  const size_t lds = (size_t)(RS_TO + span) * sizeof(double);
  const dim3 grid((unsigned)p.ntiles, (unsigned)B);
  if (L == 1) hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_TO), lds, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_TO), lds, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_segment(const float* x, int64_t x_bs, const int32_t* n, int32_t B, int32_t T, const void* tile_sq, int32_t ntiles,
                            const int32_t* start, const float* aug_gain, const float* aug_sign, const float* noise, int64_t noise_bs,
                            double noise_scale, int32_t normalize, double normalization_db, int32_t max_segment, int32_t S, float* y,
                            double* gain, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || S < 0 || max_segment < 0) return tdvc_fail(TDVC_EINVAL, "segment: negative size");
  if (max_segment > S) return tdvc_fail(TDVC_EINVAL, "segment: max_segment exceeds the output length S");
  if (max_segment == 0 && T > S) return tdvc_fail(TDVC_EINVAL, "segment: without a crop the rows must fit the output length S");
  if (B == 0 || S == 0) return TDVC_OK;
  if (!x || !n || !y) return tdvc_fail(TDVC_EINVAL, "segment: null pointer");
  if (x_bs < 0 || noise_bs < 0 || (noise && B > 1 && noise_bs < S)) return tdvc_fail(TDVC_EINVAL, "segment: bad row stride");
  if (tile_sq && ntiles < (T + RS_TO - 1) / RS_TO) return tdvc_fail(TDVC_EINVAL, "segment: fewer tile sums than the rows have tiles");
  SegmentP p;
  p.x = x; p.x_bs = x_bs; p.n = n; p.T = T; p.tile_sq = (const double*)tile_sq; p.ntiles = ntiles;
  p.start = start; p.aug_gain = aug_gain; p.aug_sign = aug_sign; p.noise = noise; p.noise_bs = noise_bs; p.noise_scale = noise_scale;
  p.target = normalize ? pow(10.0, normalization_db / 20.0) : 0.0;
  p.max_segment = max_segment; p.S = S; p.y = y; p.gain = gain;
  hipLaunchKernelGGL(segment_kernel, dim3((unsigned)B), dim3(SEG_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
