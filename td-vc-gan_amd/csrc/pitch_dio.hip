// WORLD's DIO F0 estimator and its StoneMask refinement (M. Morise et al.; WORLD's dio.cpp, stonemask.cpp, matlabfunctions.cpp as
// pyworld.dio / pyworld.stonemask call them with their defaults; the first step of the reference's objective evaluation,
// test_scripts/common/test_mcd.py world_analyze), restated in include/tdvc.h. Float64 throughout, one rounding to fp32 at the store.
//
// tdvc_dio is seven launches on one stream, none of which waits for the host:
//   dio_tables_kernel      1 + nb blocks: the low-cut FIR h (2c + 1 taps, its sum in a fixed order) and the nb Nuttall windows
//   dio_mean_kernel        one block per row: the row mean; per-thread partials in ascending order, a shuffle butterfly per wave, the 4
//                          wave sums added pairwise (reduce.h)
//   dio_lowcut_kernel      (tile, row): y = (x - mean) * h, a tile of 1024 outputs and its halo in LDS, 4 consecutive outputs per thread
//   dio_band_kernel<0>     (tile, band, row): f = y * w_k for 1024 samples with the 4 hal - 1 halo in LDS, then the four kinds of
//                          events of the tile's first 1022 samples (an event reads f[i .. i + 2]) are COUNTED (at most 511 of a
//                          kind: a crossing needs g[i] > 0 >= g[i+1])
//   dio_band_kernel<1>     the same f again, bit for bit (same code, same order); each block adds the counts of the tiles before it
//                          (integers: any order) and writes its events behind them, in order, so that the events of one (row, band,
//                          kind) are contiguous. Filtering twice costs 1408 fma per sample; storing f or per-tile event slots
//                          instead would add half as much workspace again or double it
//   dio_candidate_kernel   (256 frames, band, row): four binary searches and interpolations per frame, candidate and score
//   dio_fix_kernel         one wave per row: the best candidate per frame and steps 1 and 2 across the lanes, the section ends
//                          compacted in order with ballots, steps 3 and 4 walked by lane 0 (a serial recurrence over at most F frames)
// What bounds them: the two FIR kernels are 4 G fma in float64 at the MCD batch (16 x 4.48 s) and bound by LDS reads, which is why
// dio_fir4 keeps a sliding window of the input in registers: 4 sample reads and 4 broadcast tap reads per 16 fma, where the plain
// loop (one sample per fma) measured 1.45 ms for `dio` at that batch. Everything else is latency: the candidate kernel's 4 x ~10
// dependent probes, the fix kernel's serial walk.
// LDS: four phases of (1024 + taps)/4 doubles (rounded up) plus the taps, and 1024 doubles of f for a band: 19 KB for the low-cut and at
// most 23 KB for a band at 16 kHz (the lowest band), 50 KB at the 2048-tap limit: at least 3 blocks of 256 threads per CU, 6 or more
// at the MCD settings.
//
// tdvc_stonemask is one launch, one block of 256 threads per frame: the window's samples (fp32, as stored) and the Blackman window
// in LDS, then the at most 2 + 6 DFT bins the refinement reads by direct summation, the phase reduced exactly as (idx n) mod N in
// integers before sincospi. Two reductions of at most 24 sums, in the fixed order above.
// Every loop is bounded by the launch arguments; nothing at or past a row's length is read. No atomics: bit-identical from call to call.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include "reduce.h"

namespace tdvc {

constexpr int DIO_THREADS = 256, DIO_TS = 1024, DIO_EV = DIO_TS - 2, DIO_CAP = DIO_TS / 2;      // f samples and event samples per tile
constexpr int DIO_MAX_TAPS = 2048, DIO_MAX_BANDS = 16, DIO_MAX_T = 1 << 21;
constexpr int SM_MAX_WIN = 4096;
constexpr double DIO_EPS = 1e-12, DIO_BIG = 100000.0;

struct DioP {
  const float* x; long x_bs, x_ts;
  const int* lengths; int T, F, hop;
  double fs, f0_floor, f0_ceil, allowed;
  int nb, c, vrm, ntiles;
  int hal[DIO_MAX_BANDS], woff[DIO_MAX_BANDS];
  double bf[DIO_MAX_BANDS];
  double *mean, *h, *w, *y, *ev, *cand, *score, *sx, *sy;      // workspace
  int *counts, *totals, *neg, *pos;
  double *cand_out, *score_out;
  float* f0; long f0_bs;
};

__device__ __forceinline__ int dio_len(const DioP& p, int b) { return row_len(p.lengths, b, p.T); }

// sum over the block of 256 threads in every thread; red holds 4 doubles. The barrier before the write protects an earlier use of red.
__device__ __forceinline__ double dio_block_sum(double v, double* red, int t) {
  v = wave_sum(v);
  __syncthreads();
  block_stage(v, red, t);
  return sum_pairwise(red);
}

__global__ __launch_bounds__(DIO_THREADS) void dio_tables_kernel(DioP p) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {
    const int n = 2 * p.c + 1;
    double part = 0.0;
    for (int i = t; i < n; i += DIO_THREADS) {
      const double v = 0.5 - 0.5 * cospi((double)(i + 1) / (double)(p.c + 1));
      p.h[i] = v;
      part += v;
    }
    const double sum = dio_block_sum(part, red, t);
    for (int i = t; i < n; i += DIO_THREADS) p.h[i] = -p.h[i] / sum + (i == p.c ? 1.0 : 0.0);
  } else {
    const int k = blockIdx.x - 1, n = 4 * p.hal[k];
    double* w = p.w + p.woff[k];
    for (int i = t; i < n; i += DIO_THREADS) {
      const double u = (double)i / (double)(n - 1);
      w[i] = 0.355768 - 0.487396 * cospi(2.0 * u) + 0.144232 * cospi(4.0 * u) - 0.012604 * cospi(6.0 * u);
    }
  }
}

__global__ __launch_bounds__(DIO_THREADS) void dio_mean_kernel(DioP p) {
  __shared__ double red[4];
  const int t = threadIdx.x, b = blockIdx.x, len = dio_len(p, b);
  const float* x = p.x + b * p.x_bs;
  double part = 0.0;
  for (int i = t; i < len; i += DIO_THREADS) part += (double)x[i * p.x_ts];
  const double sum = dio_block_sum(part, red, t);
  if (t == 0) p.mean[b] = len > 0 ? sum / (double)len : 0.0;
}

// The FIR of both filter kernels. The block's input lies in LDS in four phases, sample m at in[(m & 3) * Q + (m >> 2)], the taps
// cs[0 .. K4) (K4 a multiple of 4) in order. Thread t owns the four consecutive outputs 4t .. 4t + 3:
//     acc[e] = sum_j cs[j] in[4t + e + K4 - 1 - j],   j ascending, one fma each: the order of the definition.
// Four taps per step: the thread keeps the two aligned groups of four samples that its window straddles in registers and loads
// one new group per step, so 16 fma cost 4 sample reads (each lane-consecutive within its phase: conflict-free) and 4 broadcast
// tap reads, where a plain loop reads a sample per fma.
__device__ __forceinline__ void dio_fir4(const double* in, int Q, const double* cs, int K4, int t, double acc[4]) {
  const int nq = K4 >> 2;
  const double* g = in + t;
  double n0 = g[nq], n1 = g[Q + nq], n2 = g[2 * Q + nq];
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
  for (int q = nq - 1; q >= 0; --q) {
    const double s0 = g[q], s1 = g[Q + q], s2 = g[2 * Q + q], s3 = g[3 * Q + q];
    const double* c = cs + 4 * (nq - 1 - q);
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    acc[0] = fma(c0, s3, acc[0]); acc[1] = fma(c0, n0, acc[1]); acc[2] = fma(c0, n1, acc[2]); acc[3] = fma(c0, n2, acc[3]);
    acc[0] = fma(c1, s2, acc[0]); acc[1] = fma(c1, s3, acc[1]); acc[2] = fma(c1, n0, acc[2]); acc[3] = fma(c1, n1, acc[3]);
    acc[0] = fma(c2, s1, acc[0]); acc[1] = fma(c2, s2, acc[1]); acc[2] = fma(c2, s3, acc[2]); acc[3] = fma(c2, n0, acc[3]);
    acc[0] = fma(c3, s0, acc[0]); acc[1] = fma(c3, s1, acc[1]); acc[2] = fma(c3, s2, acc[2]); acc[3] = fma(c3, s3, acc[3]);
    n0 = s0; n1 = s1; n2 = s2;
  }
}

// rows of a phase for K4 taps: the DIO_TS / 4 + K4 / 4 groups a block reads, rounded up to 4 mod 16 doubles. The reads of dio_fir4
// are conflict-free for any Q; the loader's ds_write_b64 serves 16 consecutive lanes at a time, four samples of each phase, and
// with the phases 4 doubles apart modulo 16 those land on 16 different bank pairs.
__host__ __device__ __forceinline__ int dio_phase_rows(int K4) { return ((DIO_TS + K4) / 4 + 15) / 16 * 16 + 4; }

// y[i] = sum_j h[j] xc[i + c - j], j = 0 .. 2c, xc = x - mean inside [0, len) and 0 outside; written for i < len only. The taps are
// padded with zeros to a multiple of 4 (a zero tap adds nothing: the samples it meets are finite or the zeros outside the row).
__global__ __launch_bounds__(DIO_THREADS) void dio_lowcut_kernel(DioP p) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, b = blockIdx.y, len = dio_len(p, b), i0 = blockIdx.x * DIO_TS;
  if (i0 >= len) return;
  const int c = p.c, taps = 2 * c + 1, K4 = (taps + 3) & ~3, Q = dio_phase_rows(K4);
  double* xs = lds;                 // sample m is xc[i0 + c - (K4 - 1) + m]
  double* hs = lds + 4 * Q;
  const float* x = p.x + b * p.x_bs;
  const double mean = p.mean[b];
  for (int m = t; m < DIO_TS + K4; m += DIO_THREADS) {
    const long i = (long)i0 + c - (K4 - 1) + m;
    xs[(m & 3) * Q + (m >> 2)] = (i >= 0 && i < len) ? (double)x[i * p.x_ts] - mean : 0.0;
  }
  for (int j = t; j < K4; j += DIO_THREADS) hs[j] = j < taps ? p.h[j] : 0.0;
  __syncthreads();
  double acc[4];
  dio_fir4(xs, Q, hs, K4, t, acc);
  double* y = p.y + (long)b * p.T;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + 4 * t + e;
    if (i < len) y[i] = acc[e];
  }
}

// f[i] = sum_j w[j] y[i + 2 hal - j], j = 0 .. 4 hal - 1, y = 0 outside [0, len), for the DIO_TS samples from i0 = tile * DIO_EV;
// then the events of the tile's first DIO_EV samples (an event at i reads f[i .. i + 2]).
// WRITE = 0 counts them per tile, WRITE = 1 writes them behind the events of the tiles before.
template <int WRITE>
__global__ __launch_bounds__(DIO_THREADS) void dio_band_kernel(DioP p) {
  extern __shared__ double lds[];
  __shared__ unsigned long long wtot[4];
  __shared__ int pre[4][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int tile = blockIdx.x, k = blockIdx.y, b = blockIdx.z, len = dio_len(p, b), i0 = tile * DIO_EV;
  int* counts = p.counts + (((long)b * p.nb + k) * p.ntiles) * 4;
  if (i0 >= len) {                                                           // uniform: a tile past the row has no events
    if (!WRITE && t < 4) counts[tile * 4 + t] = 0;
    if (WRITE && tile == p.ntiles - 1) {
      int part[4] = {0, 0, 0, 0};
      for (int q = t; q < tile; q += DIO_THREADS)
        for (int kind = 0; kind < 4; ++kind) part[kind] += counts[q * 4 + kind];
      for (int kind = 0; kind < 4; ++kind) {
        int v = part[kind];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) pre[kind][wv] = v;
      }
      __syncthreads();
      if (t < 4) p.totals[((long)b * p.nb + k) * 4 + t] = pre[t][0] + pre[t][1] + pre[t][2] + pre[t][3];
    }
    return;
  }
  const int hal = p.hal[k], taps = 4 * hal, Q = dio_phase_rows(taps);
  double* ys = lds;                 // sample m is y[i0 - 2 hal + 1 + m]
  double* wsm = lds + 4 * Q;
  double* fsm = wsm + taps;         // fsm[o] = f[i0 + o], o < DIO_TS
  const double* y = p.y + (long)b * p.T;
  const double* w = p.w + p.woff[k];
  for (int m = t; m < DIO_TS + taps; m += DIO_THREADS) {
    const long i = (long)i0 - 2 * hal + 1 + m;
    ys[(m & 3) * Q + (m >> 2)] = (i >= 0 && i < len) ? y[i] : 0.0;
  }
  for (int j = t; j < taps; j += DIO_THREADS) wsm[j] = w[j];
  __syncthreads();
  {
    double acc[4];
    dio_fir4(ys, Q, wsm, taps, t, acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) fsm[4 * t + e] = acc[e];
  }
  __syncthreads();

  // thread t looks at samples i0 + 4t .. i0 + 4t + 3, in order; kinds: f, -f, -(f[i+1] - f[i]), f[i+1] - f[i]
  constexpr int S = DIO_TS / DIO_THREADS;
  double fine[4][2];
  int cnt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int o = t * S + s, i = i0 + o;
    if (o >= DIO_EV) break;                                                  // the last two samples belong to the next tile
    const double f0v = fsm[o], f1v = fsm[o + 1], f2v = fsm[o + 2];
    const double d0 = f1v - f0v, d1 = f2v - f1v;
    const double g0[4] = {f0v, -f0v, -d0, d0}, g1[4] = {f1v, -f1v, -d1, d1};
#pragma unroll
    for (int kind = 0; kind < 4; ++kind) {
      const bool in = kind < 2 ? i + 1 < len : i + 2 < len;
      if (in && 0.0 < g0[kind] && g1[kind] <= 0.0) {
        const double v = (double)(i + 1) - g0[kind] / (g1[kind] - g0[kind]);
        if (cnt[kind] == 0) fine[kind][0] = v; else fine[kind][1] = v;      // at most 2 in 4 consecutive samples
        ++cnt[kind];
      }
    }
  }
  // exclusive scan over the block of the four counts, 16 bits each
  const unsigned long long mine = (unsigned long long)cnt[0] | ((unsigned long long)cnt[1] << 16) | ((unsigned long long)cnt[2] << 32) |
                                  ((unsigned long long)cnt[3] << 48);
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wtot[wv] = incl;
  __syncthreads();
  unsigned long long excl = incl - mine;
  for (int q = 0; q < wv; ++q) excl += wtot[q];
  if (!WRITE) {
    if (t == DIO_THREADS - 1) {
      const unsigned long long tot = excl + mine;
      for (int kind = 0; kind < 4; ++kind) counts[tile * 4 + kind] = (int)((tot >> (16 * kind)) & 0xffff);
    }
    return;
  }
  int part[4] = {0, 0, 0, 0};
  for (int q = t; q < tile; q += DIO_THREADS)
    for (int kind = 0; kind < 4; ++kind) part[kind] += counts[q * 4 + kind];
  for (int kind = 0; kind < 4; ++kind) {
    int v = part[kind];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) pre[kind][wv] = v;
  }
  __syncthreads();
  const long cap = (long)p.ntiles * DIO_CAP;
#pragma unroll
  for (int kind = 0; kind < 4; ++kind) {
    const int before = pre[kind][0] + pre[kind][1] + pre[kind][2] + pre[kind][3];
    const int at = before + (int)((excl >> (16 * kind)) & 0xffff);
    double* ev = p.ev + (((long)b * p.nb + k) * 4 + kind) * cap;
    if (cnt[kind] > 0 && at < cap) ev[at] = fine[kind][0];
    if (cnt[kind] > 1 && at + 1 < cap) ev[at + 1] = fine[kind][1];
    if (tile == p.ntiles - 1 && t == DIO_THREADS - 1)
      p.totals[((long)b * p.nb + k) * 4 + kind] = at + cnt[kind];
  }
}

// WORLD's histc + interp1 on the intervals of one event list: n = cnt - 1 >= 3 intervals, location (a + b)/2/fs, value fs/(b - a)
__device__ __forceinline__ double dio_interp(const double* ev, int n, double fs, double tq) {
  int lo = 0, hi = n;                                                        // the number of locations <= tq
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((ev[mid] + ev[mid + 1]) / 2.0 / fs <= tq) lo = mid + 1; else hi = mid;
  }
  const int k = min(max(lo, 1), n - 1);
  const double a = ev[k - 1], m = ev[k], z = ev[k + 1];
  const double x0 = (a + m) / 2.0 / fs, x1 = (m + z) / 2.0 / fs, y0 = fs / (m - a), y1 = fs / (z - m);
  const double s = (tq - x0) / (x1 - x0);
  return y0 + s * (y1 - y0);
}

__global__ __launch_bounds__(DIO_THREADS) void dio_candidate_kernel(DioP p) {
  const int fr = blockIdx.x * DIO_THREADS + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
  if (fr >= p.F) return;
  const int len = dio_len(p, b), Fb = min(len / p.hop + 1, p.F);
  const long cap = (long)p.ntiles * DIO_CAP;
  const int* tot = p.totals + ((long)b * p.nb + k) * 4;
  int n[4];
  bool ok = fr < Fb && p.ntiles > 0;                                         // without samples there are no totals either
  for (int kind = 0; ok && kind < 4; ++kind) {
    n[kind] = min(tot[kind], (int)cap) - 1;
    ok = n[kind] > 2;
  }
  double cand = 0.0, score = DIO_BIG / DIO_EPS;
  if (ok) {
    const double tq = (double)((long)fr * p.hop) / p.fs;
    double v[4];
    for (int kind = 0; kind < 4; ++kind) v[kind] = dio_interp(p.ev + (((long)b * p.nb + k) * 4 + kind) * cap, n[kind], p.fs, tq);
    cand = (((v[0] + v[1]) + v[2]) + v[3]) / 4.0;
    double q = 0.0;
    for (int kind = 0; kind < 4; ++kind) q += (v[kind] - cand) * (v[kind] - cand);
    score = sqrt(q / 3.0);
    const double bf = p.bf[k];
    if (cand > bf || cand < bf / 2.0 || cand > p.f0_ceil || cand < p.f0_floor) { cand = 0.0; score = DIO_BIG; }
    score /= cand + DIO_EPS;
  }
  const long at = ((long)b * p.nb + k) * p.F + fr;
  p.cand[at] = cand; p.score[at] = score;
  if (p.cand_out) p.cand_out[at] = cand;
  if (p.score_out) p.score_out[at] = score;
}

// the candidate of frame fr nearest to ref = (3 cur - past)/2 over the bands, the lowest band on a tie; 0 beyond the allowed range
__device__ __forceinline__ double dio_select(const double* cand, int nb, long F, int fr, double cur, double past, double allowed) {
  const double ref = (cur * 3.0 - past) / 2.0;
  double best = cand[fr], err = fabs(ref - best);
  for (int k = 1; k < nb; ++k) {
    const double v = cand[k * F + fr], e = fabs(ref - v);
    if (e < err) { err = e; best = v; }
  }
  return fabs(1.0 - best / ref) > allowed ? 0.0 : best;
}

__global__ __launch_bounds__(64) void dio_fix_kernel(DioP p) {
  const int b = blockIdx.x, lane = threadIdx.x, F = p.F;
  const int len = dio_len(p, b), Fb = min(len / p.hop + 1, F);
  float* out = p.f0 + b * p.f0_bs;
  const int vrm = p.vrm, c = (vrm - 1) / 2, nb = p.nb;
  if (Fb <= vrm) {
    for (int fr = lane; fr < F; fr += 64) out[fr] = 0.0f;
    return;
  }
  const double* cand = p.cand + (long)b * nb * F;
  const double* score = p.score + (long)b * nb * F;
  double* X = p.sx + (long)b * F;
  double* Y = p.sy + (long)b * F;
  int* neg = p.neg + (long)b * F;
  int* pos = p.pos + (long)b * F;
  for (int i = lane; i < Fb; i += 64) {                                      // best -> base
    double bs = score[i], bv = cand[i];
    for (int k = 1; k < nb; ++k) {
      const double s = score[(long)k * F + i];
      if (s < bs) { bs = s; bv = cand[(long)k * F + i]; }
    }
    X[i] = (i < vrm || i >= Fb - vrm) ? 0.0 : bv;
  }
  __syncthreads();
  for (int i = lane; i < Fb; i += 64)                                        // step 1
    Y[i] = i < vrm ? 0.0 : (fabs((X[i] - X[i - 1]) / (DIO_EPS + X[i])) < p.allowed ? X[i] : 0.0);
  __syncthreads();
  for (int i = lane; i < Fb; i += 64) {                                      // step 2 -> X
    double v = Y[i];
    if (i >= c && i < Fb - c)
      for (int d = -c; d <= c; ++d)
        if (Y[i + d] == 0.0) v = 0.0;
    X[i] = v;
  }
  __syncthreads();
  int nneg = 0, npos = 0;                                                    // the section ends, in order
  for (int base = 1; base < Fb; base += 64) {
    const int i = base + lane;
    const bool in = i < Fb;
    const double cur = in ? X[i] : 0.0, prev = in ? X[i - 1] : 0.0;
    const bool isneg = in && cur == 0.0 && prev != 0.0, ispos = in && prev == 0.0 && cur != 0.0;
    const unsigned long long mn = __ballot(isneg), mp = __ballot(ispos), below = (1ull << lane) - 1ull;
    if (isneg) neg[nneg + __popcll(mn & below)] = i - 1;
    if (ispos) pos[npos + __popcll(mp & below)] = i;
    nneg += __popcll(mn); npos += __popcll(mp);
  }
  __syncthreads();
  if (lane == 0) {
    for (int n = 0; n < nneg; ++n) {                                         // step 3, forward
      const int lim = n == nneg - 1 ? Fb - 1 : neg[n + 1];
      for (int j = neg[n]; j < lim; ++j) {
        const double v = dio_select(cand, nb, F, j + 1, X[j], X[max(j - 1, 0)], p.allowed);
        X[j + 1] = v;
        if (v == 0.0) break;
      }
    }
    for (int n = npos - 1; n >= 0; --n) {                                    // step 4, backward
      const int lim = n == 0 ? 1 : pos[n - 1];
      for (int j = pos[n]; j > lim; --j) {
        const double v = dio_select(cand, nb, F, j - 1, X[j], X[min(j + 1, Fb - 1)], p.allowed);
        X[j - 1] = v;
        if (v == 0.0) break;
      }
    }
  }
  __syncthreads();
  for (int fr = lane; fr < F; fr += 64) out[fr] = fr < Fb ? (float)X[fr] : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------ StoneMask
struct SmP {
  const float* x; long x_bs, x_ts;
  const int* lengths; int T;
  const float* fi; long fi_bs, fi_fs;
  int F, hop; double fs;
  float* fo; long fo_bs;
};

struct SmLds {
  float xs[SM_MAX_WIN];
  double mw[SM_MAX_WIN];
  double red[4][24];
};

// sum_h amp IF / (sum_h amp h + eps) over the harmonics h = 1 .. nh of g, from direct DFT sums at the bins idx_h; every thread
// returns the same value. N is a power of two.
__device__ double sm_fix(SmLds& s, int t, int wl, int N, double fs, double g, int nh) {
  int idx[6];
  double acc[6][4];
#pragma unroll
  for (int h = 0; h < 6; ++h) {
    idx[h] = h < nh ? (int)(g * N / fs * (h + 1) + 0.5) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[h][q] = 0.0;
  }
  for (int n = t; n < wl; n += DIO_THREADS) {
    const double xv = (double)s.xs[n];
    const double up = n + 1 < wl ? s.mw[n + 1] : 0.0, dn = n > 0 ? s.mw[n - 1] : 0.0;
    const double a = xv * s.mw[n], d = xv * (-(up - dn) / 2.0);
#pragma unroll
    for (int h = 0; h < 6; ++h) {                                            // unrolled with a guard: the sums stay in registers
      if (h < nh) {
        const long m = ((long)idx[h] * n) & (N - 1);
        double sn, cs;
        sincospi(-2.0 * (double)m / (double)N, &sn, &cs);
        acc[h][0] = fma(a, cs, acc[h][0]); acc[h][1] = fma(a, sn, acc[h][1]);
        acc[h][2] = fma(d, cs, acc[h][2]); acc[h][3] = fma(d, sn, acc[h][3]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 6; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = wave_sum(acc[h][q]);
      if ((t & 63) == 0) s.red[t >> 6][h * 4 + q] = v;
    }
  __syncthreads();
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int h = 0; h < 6; ++h) {
    if (h >= nh) break;
    double r[4];
    for (int q = 0; q < 4; ++q) r[q] = sum_pairwise<24>(&s.red[0][h * 4 + q]);
    const double P = r[0] * r[0] + r[1] * r[1], nm = r[0] * r[3] - r[1] * r[2];
    const double inst = P == 0.0 ? 0.0 : (double)idx[h] * fs / N + nm / P * fs / 2.0 / M_PI;
    const double amp = sqrt(P);
    num += amp * inst; den += amp * (h + 1);
  }
  return num / (den + DIO_EPS);
}

__global__ __launch_bounds__(DIO_THREADS) void stonemask_kernel(SmP p) {
  __shared__ SmLds s;
  const int t = threadIdx.x;
  const long blk = blockIdx.x;
  const long b = blk / p.F, fr = blk - b * p.F;
  const float fv = p.fi[b * p.fi_bs + fr * p.fi_fs];
  float* o = p.fo + b * p.fo_bs + fr;
  const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;   // row_len, spelled out: as a call the test below compiles differently
  const double fs = p.fs, f = (double)fv;
  if (!isfinite(fv) || f <= 40.0 || f > fs / 12.0 || len <= 0) {             // uniform over the block
    if (t == 0) *o = 0.0f;
    return;
  }
  const int half = min((int)(1.5 * fs / f + 1.0), (SM_MAX_WIN - 1) / 2), wl = 2 * half + 1;
  const int N = 1 << (2 + (31 - __clz(wl)));
  const double tt = (double)(fr * p.hop) / fs;
  const float* x = p.x + b * p.x_bs;
  for (int n = t; n < wl; n += DIO_THREADS) {
    const int k = n - half;
    const double v = (tt + (double)k / fs) * fs + 0.001;
    const long raw = v > 0.0 ? (long)(v + 0.5) : (long)(v - 0.5);
    s.xs[n] = x[min(max(raw - 1, 0L), (long)len - 1) * p.x_ts];
    const double u = (((double)raw - 1.0) / fs - tt) / ((2.0 * half + 1.0) / fs);
    s.mw[n] = 0.42 + 0.5 * cospi(2.0 * u) + 0.08 * cospi(4.0 * u);
  }
  __syncthreads();
  const double tent = sm_fix(s, t, wl, N, fs, f, 2);
  double r = 0.0;
  if (!(tent <= 0.0 || tent > f * 2.0)) r = sm_fix(s, t, wl, N, fs, tent, min((int)(fs / 2.0 / f), 6));      // uniform: every thread holds the same tent
  if (fabs(r - f) > 0.2 * f) r = f;
  if (t == 0) *o = (float)r;
}

// ------------------------------------------------------------------------------------------------------------ host
struct DioPlan {
  int nb, c, vrm, ntiles, wtaps;
  int hal[DIO_MAX_BANDS], woff[DIO_MAX_BANDS];
  double bf[DIO_MAX_BANDS];
  size_t off_mean, off_h, off_w, off_y, off_ev, off_cand, off_score, off_sx, off_sy, off_counts, off_totals, off_neg, off_pos, bytes;
};

static int dio_round(double v) { return (int)(v + 0.5); }

static int dio_num_bands(double f0_floor, double f0_ceil, double cpo) {
  if (!(f0_floor > 0.0) || !(f0_ceil > f0_floor) || !(cpo > 0.0) || !isfinite(f0_ceil) || !isfinite(cpo)) return 0;
  const double v = 1.0 + floor(log2(f0_ceil / f0_floor) * cpo);
  return v > 1e6 ? 1000000 : (int)v;
}

// the argument checks of tdvc_dio that do not involve pointers; fills the plan when they pass
static int dio_plan(int32_t B, int32_t T, int32_t F, int32_t hop, int32_t fs, double f0_floor, double f0_ceil, double cpo, DioPlan* pl) {
  if (B < 0 || T < 0 || F < 0) return tdvc_fail(TDVC_EINVAL, "dio: negative batch, sample or frame count");
  if (hop < 1 || fs < 1) return tdvc_fail(TDVC_EINVAL, "dio: hop and fs must be positive");
  const int nb = dio_num_bands(f0_floor, f0_ceil, cpo);
  if (nb < 1) return tdvc_fail(TDVC_EINVAL, "dio: needs 0 < f0_floor < f0_ceil and channels_in_octave > 0, all finite");
  if (nb > DIO_MAX_BANDS) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: more than 16 bands");
  if (T > DIO_MAX_T) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: more than 2^21 samples per row");
  if (B > 65535) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: more than 65535 rows");
  pl->nb = nb;
  pl->c = dio_round(fs / 50.0);
  if (2 * pl->c + 1 > DIO_MAX_TAPS) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: the low-cut filter of this fs has more than 2048 taps");
  pl->wtaps = 0;
  for (int k = 0; k < nb; ++k) {
    pl->bf[k] = f0_floor * pow(2.0, (k + 1) / cpo);
    const double hv = fs / pl->bf[k] / 2.0;
    if (!(hv + 0.5 >= 1.0)) return tdvc_fail(TDVC_EINVAL, "dio: a band at or above fs: lower f0_ceil");
    if (4.0 * hv > DIO_MAX_TAPS) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: the lowest band's filter has more than 2048 taps: raise f0_floor");
    pl->hal[k] = dio_round(hv);
    if (4 * pl->hal[k] > DIO_MAX_TAPS) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: the lowest band's filter has more than 2048 taps: raise f0_floor");
    pl->woff[k] = pl->wtaps;
    pl->wtaps += 4 * pl->hal[k];
  }
  const double vr = 0.5 + (double)fs / hop / f0_floor;
  if (vr > 1e6) return tdvc_fail(TDVC_EUNSUPPORTED, "dio: fs / hop / f0_floor above 10^6");
  pl->vrm = (int)vr * 2 + 1;
  pl->ntiles = (T + DIO_EV - 1) / DIO_EV;
  size_t at = 0;
  auto take = [&](size_t n) { const size_t o = at; at += (n + 63) / 64 * 64; return o; };
  const size_t b = (size_t)B, rows = b * nb;
  pl->off_mean = take(b * 8);
  pl->off_h = take((size_t)(2 * pl->c + 1) * 8);
  pl->off_w = take((size_t)pl->wtaps * 8);
  pl->off_y = take(b * T * 8);
  pl->off_ev = take(rows * 4 * pl->ntiles * DIO_CAP * 8);
  pl->off_cand = take(rows * F * 8);
  pl->off_score = take(rows * F * 8);
  pl->off_sx = take(b * F * 8);
  pl->off_sy = take(b * F * 8);
  pl->off_counts = take(rows * pl->ntiles * 4 * 4);
  pl->off_totals = take(rows * 4 * 4);
  pl->off_neg = take(b * F * 4);
  pl->off_pos = take(b * F * 4);
  pl->bytes = at;
  return TDVC_OK;
}

}  // namespace tdvc

extern "C" int32_t tdvc_dio_num_bands(double f0_floor, double f0_ceil, double channels_in_octave) {
  const int nb = tdvc::dio_num_bands(f0_floor, f0_ceil, channels_in_octave);
  return nb > tdvc::DIO_MAX_BANDS ? 0 : nb;
}

extern "C" size_t tdvc_dio_workspace(int32_t B, int32_t T, int32_t F, int32_t hop, int32_t fs, double f0_floor, double f0_ceil,
                                     double channels_in_octave) {
  tdvc::DioPlan pl;
  if (tdvc::dio_plan(B, T, F, hop, fs, f0_floor, f0_ceil, channels_in_octave, &pl) != TDVC_OK) return 0;
  if (B == 0 || F == 0 || F < T / hop + 1) return 0;
  return pl.bytes;
}

extern "C" int tdvc_dio(const float* signal, int64_t s_bs, int64_t s_ts, const int32_t* lengths, int32_t T, int32_t B, int32_t F, int32_t hop,
                        int32_t fs, double f0_floor, double f0_ceil, double channels_in_octave, double allowed_range, float* f0,
                        int64_t f0_bs, double* cand, double* score, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  DioPlan pl;
  const int rc = dio_plan(B, T, F, hop, fs, f0_floor, f0_ceil, channels_in_octave, &pl);
  if (rc != TDVC_OK) return rc;
  if (!(allowed_range > 0.0) || !isfinite(allowed_range)) return tdvc_fail(TDVC_EINVAL, "dio: allowed_range must be positive and finite");
  if (s_bs < 0 || s_ts < 0 || f0_bs < 0) return tdvc_fail(TDVC_EINVAL, "dio: negative stride");
  if (B == 0 || F == 0) return TDVC_OK;
  if (F < T / hop + 1) return tdvc_fail(TDVC_EINVAL, "dio: F must hold the T / hop + 1 frames of a full row");
  if (B > 1 && f0_bs < F) return tdvc_fail(TDVC_EINVAL, "dio: overlapping f0 rows");
  if ((!signal && T > 0) || !f0) return tdvc_fail(TDVC_EINVAL, "dio: null pointer");
  if (!workspace || workspace_bytes < pl.bytes) return tdvc_fail(TDVC_EWORKSPACE, "dio: workspace is null or smaller than tdvc_dio_workspace");
  char* ws = (char*)workspace;
  DioP p;
  p.x = signal; p.x_bs = s_bs; p.x_ts = s_ts; p.lengths = lengths; p.T = T; p.F = F; p.hop = hop;
  p.fs = fs; p.f0_floor = f0_floor; p.f0_ceil = f0_ceil; p.allowed = allowed_range;
  p.nb = pl.nb; p.c = pl.c; p.vrm = pl.vrm; p.ntiles = pl.ntiles;
  for (int k = 0; k < DIO_MAX_BANDS; ++k) {
    p.hal[k] = k < pl.nb ? pl.hal[k] : 1; p.woff[k] = k < pl.nb ? pl.woff[k] : 0; p.bf[k] = k < pl.nb ? pl.bf[k] : 0.0;
  }
  p.mean = (double*)(ws + pl.off_mean); p.h = (double*)(ws + pl.off_h); p.w = (double*)(ws + pl.off_w); p.y = (double*)(ws + pl.off_y);
  p.ev = (double*)(ws + pl.off_ev); p.cand = (double*)(ws + pl.off_cand); p.score = (double*)(ws + pl.off_score);
  p.sx = (double*)(ws + pl.off_sx); p.sy = (double*)(ws + pl.off_sy); p.counts = (int*)(ws + pl.off_counts);
  p.totals = (int*)(ws + pl.off_totals); p.neg = (int*)(ws + pl.off_neg); p.pos = (int*)(ws + pl.off_pos);
  p.cand_out = cand; p.score_out = score; p.f0 = f0; p.f0_bs = f0_bs;
  hipStream_t st = (hipStream_t)stream;
  TDVC_TRACE(dio_tables_kernel);
  hipLaunchKernelGGL(dio_tables_kernel, dim3(1 + pl.nb), dim3(DIO_THREADS), 0, st, p);
  TDVC_TRACE(dio_mean_kernel);
  hipLaunchKernelGGL(dio_mean_kernel, dim3(B), dim3(DIO_THREADS), 0, st, p);
  if (T > 0) {
    const int k4 = (2 * pl.c + 1 + 3) & ~3;
    const size_t lc = (size_t)(4 * dio_phase_rows(k4) + k4) * 8;
    TDVC_TRACE(dio_lowcut_kernel);
    hipLaunchKernelGGL(dio_lowcut_kernel, dim3((T + DIO_TS - 1) / DIO_TS, B), dim3(DIO_THREADS), lc, st, p);
    const size_t lb = (size_t)(4 * dio_phase_rows(4 * pl.hal[0]) + 4 * pl.hal[0] + DIO_TS) * 8;      // band 0 has the longest filter
    TDVC_TRACE(dio_band_kernel<0>);
    hipLaunchKernelGGL(dio_band_kernel<0>, dim3(pl.ntiles, pl.nb, B), dim3(DIO_THREADS), lb, st, p);
    TDVC_TRACE(dio_band_kernel<1>);
    hipLaunchKernelGGL(dio_band_kernel<1>, dim3(pl.ntiles, pl.nb, B), dim3(DIO_THREADS), lb, st, p);
    TDVC_TRACE(dio_candidate_kernel);
    hipLaunchKernelGGL(dio_candidate_kernel, dim3((F + DIO_THREADS - 1) / DIO_THREADS, pl.nb, B), dim3(DIO_THREADS), 0, st, p);
  }
  TDVC_TRACE(dio_fix_kernel);
  hipLaunchKernelGGL(dio_fix_kernel, dim3(B), dim3(64), 0, st, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_stonemask(const float* signal, int64_t s_bs, int64_t s_ts, const int32_t* lengths, int32_t T, const float* f0_in,
                              int64_t fi_bs, int64_t fi_fs, int32_t B, int32_t F, int32_t hop, int32_t fs, float* f0_out, int64_t fo_bs,
                              void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0 || T < 0) return tdvc_fail(TDVC_EINVAL, "stonemask: negative batch, frame or sample count");
  if (hop < 1 || fs < 1) return tdvc_fail(TDVC_EINVAL, "stonemask: hop and fs must be positive");
  if (s_bs < 0 || s_ts < 0 || fi_bs < 0 || fi_fs < 0 || fo_bs < 0) return tdvc_fail(TDVC_EINVAL, "stonemask: negative stride");
  if (2 * (int64_t)(1.5 * fs / 40.0 + 1.0) + 1 > SM_MAX_WIN)
    return tdvc_fail(TDVC_EUNSUPPORTED, "stonemask: the window of a 40 Hz frame at this fs has more than 4096 samples");
  if ((int64_t)B * F > 0x7fffffff) return tdvc_fail(TDVC_EUNSUPPORTED, "stonemask: more than 2^31 - 1 frames");
  if ((int64_t)F * hop > 0x7fffffff) return tdvc_fail(TDVC_EUNSUPPORTED, "stonemask: frames past sample 2^31 - 1");
  if (B == 0 || F == 0) return TDVC_OK;
  if (B > 1 && fo_bs < F) return tdvc_fail(TDVC_EINVAL, "stonemask: overlapping output rows");
  if ((!signal && T > 0) || !f0_in || !f0_out) return tdvc_fail(TDVC_EINVAL, "stonemask: null pointer");
  SmP p;
  p.x = signal; p.x_bs = s_bs; p.x_ts = s_ts; p.lengths = lengths; p.T = T; p.fi = f0_in; p.fi_bs = fi_bs; p.fi_fs = fi_fs;
  p.F = F; p.hop = hop; p.fs = fs; p.fo = f0_out; p.fo_bs = fo_bs;
  TDVC_TRACE(stonemask_kernel);
  hipLaunchKernelGGL(stonemask_kernel, dim3((unsigned)((int64_t)B * F)), dim3(DIO_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
