// WORLD's CheapTrick spectral envelope (Morise 2015; the pyworld.cheaptrick(signal, f0, time_axis, sr, fft_size) step of the
// reference's objective evaluation, test_scripts/common/test_mcd.py world_analyze), restated in include/tdvc.h, and the mel-cepstrum
// of that envelope without leaving the block.
//
// tdvc_cheaptrick: one launch, one block of 256 threads per frame, the frame in LDS from the window to the output, float64
// throughout and one rounding to fp32 at the store. With N = n_fft and h = N/2 a block holds
//     A    [N]        the packed complex work array of the transforms (re = A[0 .. h), im = A[h .. N)); between the first and
//                     the second transform the mirrored spectrum and its running sum (at most 5N/6 + 3 values)
//     tw   [h + h/4]  twiddles from sincospi in double: exp(-2 pi i k/N), k < h, for the real-input split and the two widest
//                     butterfly stages, then one dense run exp(-pi i pos/m), pos < m, per narrower stage m = 1 .. h/8
//     P, R [h + 1]    power spectrum, later the liftered cepstrum c; log of the smoothed spectrum
// 53 KB at N = 2048, 27 KB at 1024: 3 and 5 blocks per CU.
//   window     thread t owns samples t, t + 256, ... of the (at most N - 3) window samples in registers; sum w^2, sum x w, sum w:
//              per-thread partials in ascending order, a shuffle butterfly per wave, the 4 wave sums added pairwise (reduce.h)
//   transform  a real sequence of N points is packed as h complex points z[j] = v[2j] + i v[2j+1] in bit-reversed order, h/2
//              in-place radix-2 butterflies per stage (log2 h stages, one barrier each), then the split X[k] = E[k] + w^k O[k].
//              The lanes of a wave touch 32 values out of 64 consecutive ones (stages m < 32: 2-way on the 64-bit banks) or 32
//              consecutive ones, and every stage with m <= h/8 reads its twiddles from a dense run; a single table would be read
//              with a stride of h/m doubles, all 32 lanes of a group on one bank pair at m = 32
//   smoothing  the DC-corrected, mirrored spectrum times df goes into A, thread t sums its N/256 consecutive values, the 256
//              totals are scanned by shuffles per wave and the 4 wave totals added in order; S from two interpolated reads
//   lifter     log S extended evenly -> transform -> c[n] = C[n] sinc lifter / N into P
//   mc         the loop of tdvc_sp2mc (csrc/eval_mcep.hip) on c with c[0] halved: wave w owns coefficients w, w + 4, ...
//   env        c extended evenly -> transform -> exp -> store
// Every loop is bounded by N; the window length and the smoothing width derived from f0 are clamped to what the arrays hold.
// No atomics, a fixed order in every sum: bit-identical from call to call.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include "reduce.h"

namespace tdvc {

constexpr int CT_THREADS = 256;
constexpr double CT_DEFAULT_F0 = 500.0;      // WORLD's kDefaultF0: the unvoiced frame
constexpr double CT_EPS = 2.2e-16;

struct CtP {
  const float* x; long x_bs, x_ts;
  const int* lengths; int T;
  const float* f0; long f0_bs, f0_fs;
  int F, hop, fs;
  double q1, floor_;
  const double* G; int order;
  float* env; float* mc;
};

template <int N>
struct CtLds {
  static constexpr int H = N / 2, TW = H + H / 4;
  double A[N];
  double twr[TW], twi[TW];
  double P[H + 1], R[H + 1];
  double red[3][CT_THREADS / 64];
};

// v(n), n < N, real -> packed complex in bit-reversed order
template <int N, typename Fn>
__device__ __forceinline__ void ct_pack(CtLds<N>& s, int t, Fn v) {
  constexpr int H = N / 2, LOG = __builtin_ctz(H);
  for (int n = t; n < N; n += CT_THREADS) {
    const int r = (int)(__brev((unsigned)(n >> 1)) >> (32 - LOG));
    s.A[(n & 1) * H + r] = v(n);
  }
  __syncthreads();
}

// in-place radix-2 transform of the h packed points; leaves a barrier behind
template <int N>
__device__ __forceinline__ void ct_fft(CtLds<N>& s, int t) {
  constexpr int H = N / 2, LOG = __builtin_ctz(H);
  double* re = s.A;
  double* im = s.A + H;
#pragma unroll
  for (int st = 1; st <= LOG; ++st) {
    const int m = 1 << (st - 1);
    for (int j = t; j < H / 2; j += CT_THREADS) {
      const int pos = j & (m - 1);
      const int i0 = ((j >> (st - 1)) << st) | pos, i1 = i0 + m;
      const int ti = m <= H / 8 ? H + m - 1 + pos : pos * (H / m);
      const double wr = s.twr[ti], wi = s.twi[ti];
      const double br = re[i1], bi = im[i1], ar = re[i0], ai = im[i0];
      const double tr = wr * br - wi * bi, tim = wr * bi + wi * br;
      re[i1] = ar - tr; im[i1] = ai - tim;
      re[i0] = ar + tr; im[i0] = ai + tim;
    }
    __syncthreads();
  }
}

// bin k, 0 <= k <= h, of the N-point transform of the packed real sequence
template <int N>
__device__ __forceinline__ void ct_split(const CtLds<N>& s, int k, double& xr, double& xi) {
  constexpr int H = N / 2;
  const int a = k & (H - 1), b = (H - k) & (H - 1);
  const double zr = s.A[a], zi = s.A[H + a], cr = s.A[b], ci = -s.A[H + b];
  const double er = 0.5 * (zr + cr), ei = 0.5 * (zi + ci), orr = 0.5 * (zi - ci), oi = -0.5 * (zr - cr);
  const double wr = k < H ? s.twr[k] : -1.0, wi = k < H ? s.twi[k] : 0.0;
  xr = er + (wr * orr - wi * oi);
  xi = ei + (wr * oi + wi * orr);
}

__device__ __forceinline__ double ct_lin(const double* y, int last, double p) {
  const int j = min(max((int)floor(p), 0), last - 1);
  return y[j] + (y[j + 1] - y[j]) * (p - (double)j);
}

template <int N>
__global__ __launch_bounds__(CT_THREADS) void cheaptrick_kernel(CtP p) {
  constexpr int H = N / 2, E = N / CT_THREADS;
  __shared__ CtLds<N> s;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long fr = blockIdx.x;
  const long b = fr / p.F, f = fr - b * p.F;

  for (int i = t; i < CtLds<N>::TW; i += CT_THREADS) {
    double ang;
    if (i < H) {
      ang = -2.0 * i / N;
    } else {
      const int j = i - H + 1, m = 1 << (31 - __clz(j));
      ang = -(double)(j - m) / m;
    }
    sincospi(ang, &s.twi[i], &s.twr[i]);
  }

  // effective F0, window length
  const double fs = p.fs, df = fs / N;
  const float f0v = p.f0[b * p.f0_bs + f * p.f0_fs];
  double fe = (double)f0v;
  if (!isfinite(f0v) || !(fe > 3.0 * fs / (N - 3.0) && fe <= fs / 4.0)) fe = CT_DEFAULT_F0;
  const int half = min((int)floor(1.5 * fs / fe + 0.5), (N - 4) / 2);
  const int wlen = 2 * half + 1;
  const int len = row_len(p.lengths, b, p.T);
  const long pos = f * (long)p.hop;
  const float* xrow = p.x + b * p.x_bs;

  double w[E], xv[E];
  double sw2 = 0.0, sxw = 0.0, sw = 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = t + e * CT_THREADS;
    w[e] = 0.0; xv[e] = 0.0;
    if (i < wlen) {
      const int k = i - half;
      w[e] = 0.5 * cos(M_PI * fe * k / (1.5 * fs)) + 0.5;
      if (len > 0) xv[e] = (double)xrow[min(max(pos + k, 0L), (long)len - 1) * p.x_ts];
      sw2 = fma(w[e], w[e], sw2); sxw = fma(xv[e], w[e], sxw); sw += w[e];
    }
  }
  sw2 = wave_sum(sw2); sxw = wave_sum(sxw); sw = wave_sum(sw);
  if (lane == 0) { s.red[0][wv] = sw2; s.red[1][wv] = sxw; s.red[2][wv] = sw; }
  __syncthreads();
  sw2 = sum_pairwise(s.red[0]); sxw = sum_pairwise(s.red[1]); sw = sum_pairwise(s.red[2]);
  const double nrm = sqrt(sw2), mean = sxw / sw;
  {
    constexpr int LOG = __builtin_ctz(H);
#pragma unroll
    for (int e = 0; e < E; ++e) {                                          // s = x w - w mean(x), zero behind the window
      const int n = t + e * CT_THREADS;
      const double wn = w[e] / nrm;
      const int r = (int)(__brev((unsigned)(n >> 1)) >> (32 - LOG));
      s.A[(n & 1) * H + r] = xv[e] * wn - wn * mean;
    }
    __syncthreads();
  }
  ct_fft<N>(s, t);
  for (int k = t; k <= H; k += CT_THREADS) {
    double xr, xi;
    ct_split<N>(s, k, xr, xi);
    s.P[k] = xr * xr + xi * xi;
  }
  __syncthreads();

  // DC correction (from the uncorrected P), mirror, running sum
  const int ul1 = 1 + (int)floor(fe * N / fs);
  const double wd = 2.0 * fe / 3.0;
  const int bd = min((int)floor(wd * N / fs) + 1, (H - 1) / 2);
  const int ls = H + 2 * bd + 1;                                           // <= N
  double part[E];
  double run = 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = t * E + e;
    double v = 0.0;
    if (j < ls) {
      const int i = j < bd ? bd - j : (j <= bd + H ? j - bd : 2 * H + bd - j);
      v = s.P[i];
      if (i < ul1) v += ct_lin(s.P, H, (fe - i * df) / df);
      v *= df;
    }
    run += v;
    part[e] = run;
  }
  double incl = run;                                                       // inclusive scan of the 256 totals
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == 63) s.red[0][wv] = incl;
  __syncthreads();
  double base = incl - run;
  for (int k = 0; k < wv; ++k) base += s.red[0][k];
#pragma unroll
  for (int e = 0; e < E; ++e) s.A[t * E + e] = base + part[e];
  __syncthreads();

  // smoothing, safeguard, logarithm
  {
    const double off = wd / (2.0 * df);
    for (int i = t; i <= H; i += CT_THREADS) {
      const double hi = ct_lin(s.A, ls - 1, i + off + bd - 0.5), lo = ct_lin(s.A, ls - 1, i - off + bd - 0.5);
      s.R[i] = log(fmax((hi - lo) / wd, p.floor_) + CT_EPS);
    }
  }
  __syncthreads();

  // lifter: c into P
  ct_pack<N>(s, t, [&](int n) { return s.R[n <= H ? n : N - n]; });
  ct_fft<N>(s, t);
  for (int n = t; n <= H; n += CT_THREADS) {
    double cr, ci;
    ct_split<N>(s, n, cr, ci);
    const double q = n / fs;
    const double sl = n == 0 ? 1.0 : sin(M_PI * fe * q) / (M_PI * fe * q);
    const double cl = (1.0 - 2.0 * p.q1) + 2.0 * p.q1 * cos(2.0 * M_PI * fe * q);
    s.P[n] = cr * sl * cl / N;
  }
  __syncthreads();

  if (p.mc) {
    float* out = p.mc + fr * (p.order + 1);
    for (int o = wv; o <= p.order; o += CT_THREADS / 64) {
      const double* row = p.G + (long)o * (H + 1);
      double acc = 0.0;
      for (int k = lane; k <= H; k += 64) acc = fma(row[k], k == 0 ? 0.5 * s.P[0] : s.P[k], acc);
      acc = wave_sum(acc);
      if (lane == 0) out[o] = (float)acc;
    }
  }
  if (p.env) {
    ct_pack<N>(s, t, [&](int n) { return s.P[n <= H ? n : N - n]; });
    ct_fft<N>(s, t);
    float* out = p.env + fr * (H + 1);
    for (int k = t; k <= H; k += CT_THREADS) {
      double xr, xi;
      ct_split<N>(s, k, xr, xi);
      out[k] = (float)exp(xr);
    }
  }
}

template <int N>
static void ct_launch(const CtP& p, long frames, hipStream_t stream) {
  TDVC_TRACE((cheaptrick_kernel<N>));
  hipLaunchKernelGGL(cheaptrick_kernel<N>, dim3((unsigned)frames), dim3(CT_THREADS), 0, stream, p);
}

}  // namespace tdvc

extern "C" int tdvc_cheaptrick(const float* signal, int64_t s_bs, int64_t s_ts, const int32_t* lengths, int32_t T, const float* f0,
                               int64_t f0_bs, int64_t f0_fs, int32_t B, int32_t F, int32_t hop, int32_t fs, int32_t n_fft, double q1,
                               double floor_, const double* G, int32_t order, float* env, float* mc, void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0 || T < 0) return tdvc_fail(TDVC_EINVAL, "cheaptrick: negative batch, frame or sample count");
  if (hop < 1 || fs < 1) return tdvc_fail(TDVC_EINVAL, "cheaptrick: hop and fs must be positive");
  if (!(floor_ > 0.0) || isinf(floor_)) return tdvc_fail(TDVC_EINVAL, "cheaptrick: floor must be positive and finite");
  if (!isfinite(q1)) return tdvc_fail(TDVC_EINVAL, "cheaptrick: q1 must be finite");
  if (s_bs < 0 || s_ts < 0 || f0_bs < 0 || f0_fs < 0) return tdvc_fail(TDVC_EINVAL, "cheaptrick: negative stride");
  if (!env && !mc) return tdvc_fail(TDVC_EINVAL, "cheaptrick: env and mc are both null");
  if (mc && !G) return tdvc_fail(TDVC_EINVAL, "cheaptrick: mc needs the matrix G");
  if (mc && order < 0) return tdvc_fail(TDVC_EINVAL, "cheaptrick: negative order");
  if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return tdvc_fail(TDVC_EUNSUPPORTED, "cheaptrick: n_fft must be 512, 1024 or 2048");
  if (mc && order > n_fft / 2) return tdvc_fail(TDVC_EINVAL, "cheaptrick: order above n_fft/2");
  if (!(3.0 * fs / (n_fft - 3.0) < CT_DEFAULT_F0 && CT_DEFAULT_F0 <= fs / 4.0))
    return tdvc_fail(TDVC_EINVAL, "cheaptrick: fs puts the unvoiced frame's 500 Hz outside (3 fs/(n_fft - 3), fs/4]");
  if ((int64_t)B * F > 0x7fffffff) return tdvc_fail(TDVC_EUNSUPPORTED, "cheaptrick: more than 2^31 - 1 frames");
  if (B == 0 || F == 0) return TDVC_OK;
  if (!signal || !f0) return tdvc_fail(TDVC_EINVAL, "cheaptrick: null pointer");
  CtP p;
  p.x = signal; p.x_bs = s_bs; p.x_ts = s_ts; p.lengths = lengths; p.T = T; p.f0 = f0; p.f0_bs = f0_bs; p.f0_fs = f0_fs;
  p.F = F; p.hop = hop; p.fs = fs; p.q1 = q1; p.floor_ = floor_; p.G = G; p.order = order; p.env = env; p.mc = mc;
  const long frames = (long)B * F;
  if (n_fft == 512) ct_launch<512>(p, frames, (hipStream_t)stream);
  else if (n_fft == 1024) ct_launch<1024>(p, frames, (hipStream_t)stream);
  else ct_launch<2048>(p, frames, (hipStream_t)stream);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
