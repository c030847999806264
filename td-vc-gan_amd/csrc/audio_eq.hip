// Batched random parametric EQ (the reference's audio_corruption.random_eq + util.eq_rms_signals): per-row biquad cascades in
// float64, parallel over time, and the RBJ coefficient formulas of params2sos on the device.
//
// tdvc_sos_filter: one 256-thread block per row. A cascade of S biquads (transposed direct form II) is a linear system with a
// 2S-dimensional state, state[n+1] = A state[n] + B x[n], so the row is cut into 224 chunks of Lc = ceil(T / 224) samples, one
// lane each, and the serial dependence over T is broken in three steps:
//   pass 1   every chunk lane runs its chunk through all S sections from a ZERO state and keeps the end state f_c; 2S further
//            lanes (224 ...) run Lc steps on zero input from the unit states e_j, which gives the columns of M = A^Lc
//   carry    2S lanes of wave 0 propagate the true state across chunks, s_{c+1} = M s_c + f_c: one matrix row per lane, the
//            state broadcast with v_readlane (no LDS round trip on the dependent path), 224 steps at most
//   pass 2   every lane re-runs its chunk from its true start state and accumulates sum(y^2) and sum(x^2); without match_rms it
//            writes y here and the kernel ends
//   pass 3   (match_rms) after a fixed-order block reduction gives gain = rms(x) / (rms(y) + 1e-8), the chunk runs once more
//            and writes (float)(y * gain): one rounding, of the float64 product
// Everything is float64: the 60 Hz shelf and peak sections have poles at radius 0.996-0.998 at 16 kHz (1 + a1 + a2 ~ 5.6e-4),
// where fp32 coefficients or fp32 state cost 1.5e-4..3.6e-4 of the output RMS. All sections are stable, so M is a
// contraction in the long run and the carry is well behaved. Within a chunk the samples run in sample-by-section order: section
// s of sample n depends on section s-1 of sample n and section s of sample n-1 only, so up to S recurrences are in flight.
// Coefficients and state live in VGPRs (7S doubles; the section count is a template argument), x is read in blocks of 8
// samples one block ahead of its use. No atomics, a fixed summation order: two calls give identical bits. No workspace.
#include "../../include/tdvc.h"
#include "api_util.h"

namespace tdvc {

constexpr int EQ_THREADS = 256;
constexpr int EQ_MAX_S = 16;
constexpr int EQ_CHUNKS = EQ_THREADS - 2 * EQ_MAX_S;      // 224 chunk lanes; lanes 224 .. 224 + 2S - 1 run the homogeneous system
constexpr int EQ_BLK = 8;                                  // samples per register block

struct SosP {
  const float* x; long x_bs;
  const double* sos;
  int T, Lc, nfull;                                        // chunk length; chunks that have a successor (= carry steps)
  int match_rms;
  float* y; long y_bs;
};

__device__ __forceinline__ double eq_bcast(double v, int lane) {      // lane is a compile-time constant at every call
  int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

enum { EQ_STATE = 0, EQ_SUMS = 1, EQ_WRITE = 2 };

// Lc steps of the cascade on x[0 .. len) followed by zeros, from state z (updated in place). EQ_SUMS adds y^2 / x^2 of the first
// len samples to sy / sx in sample order; EQ_WRITE stores (float)(y * gain) for them.
template <int S, int MODE>
__device__ __forceinline__ void eq_run_chunk(const float* __restrict__ xr, int len, int Lc, const double (&c)[S][5], double (&z)[S][2],
                                             double& sy, double& sx, float* __restrict__ yr, double gain) {
  float cur[EQ_BLK], nxt[EQ_BLK];
#pragma unroll
  for (int k = 0; k < EQ_BLK; ++k) cur[k] = (k < len) ? xr[k] : 0.f;
  for (int n0 = 0; n0 < Lc; n0 += EQ_BLK) {
#pragma unroll
    for (int k = 0; k < EQ_BLK; ++k) {
      const int n = n0 + EQ_BLK + k;
      nxt[k] = (n < len) ? xr[n] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < EQ_BLK; ++k) {
      const int n = n0 + k;
      if (n >= Lc) break;                                  // uniform: Lc is the same in every lane
      const double xv = (double)cur[k];
      double v = xv;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const double o = c[s][0] * v + z[s][0];
        z[s][0] = c[s][1] * v - c[s][3] * o + z[s][1];
        z[s][1] = c[s][2] * v - c[s][4] * o;
        v = o;
      }
      if (MODE == EQ_SUMS) {
        sx += xv * xv;                                     // x is zero past len
        if (n < len) sy += v * v;
      }
      if (MODE == EQ_WRITE) {
        if (n < len) yr[n] = (float)(v * gain);
      }
    }
#pragma unroll
    for (int k = 0; k < EQ_BLK; ++k) cur[k] = nxt[k];
  }
}

template <int S>
__global__ __launch_bounds__(EQ_THREADS) void sos_filter_kernel(SosP p) {
  constexpr int N = 2 * S;
  // st[c]: chunk c's zero-state end state f_c, then (after the carry) the state at the START of chunk c+1. Dead once pass 2 has
  // its start states, so the block reduction reuses the space: 64 KiB in all at S = 16.
  constexpr int ST_DOUBLES = EQ_CHUNKS * N > 2 * EQ_THREADS ? EQ_CHUNKS * N : 2 * EQ_THREADS;
  __shared__ double lds[ST_DOUBLES];
  __shared__ double Mt[N][N];              // Mt[j][i] = (A^Lc)[i][j]: what unit state e_j becomes after Lc steps on zero input
  double (*st)[N] = reinterpret_cast<double (*)[N]>(lds);
  double (*red)[EQ_THREADS] = reinterpret_cast<double (*)[EQ_THREADS]>(lds);

  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const bool chunk_lane = tid < EQ_CHUNKS;
  const int hj = tid - EQ_CHUNKS;          // homogeneous lanes: the unit state they start from
  const long start = (long)tid * p.Lc;
  int len = 0;
  if (chunk_lane && start < p.T) len = (p.T - start < p.Lc) ? (int)(p.T - start) : p.Lc;
  const float* xr = p.x + b * p.x_bs + (len > 0 ? start : 0);      // dereferenced at [0, len) only
  float* yr = p.y + b * p.y_bs + (len > 0 ? start : 0);

  // The row's coefficients go through LDS into per-lane registers. Read straight from global they are wave-uniform, the compiler
  // keeps them in SGPRs, 5S doubles do not fit the 102 of them, and every use in the inner loop becomes a v_readlane from a spill
  // lane: more readlanes than FMAs at S = 10. A value loaded from LDS stays in a VGPR.
  double c[S][5];
  {
    const double* sp = p.sos + b * (long)(S * 6);
    if (tid < S * 5) {
      const int s = tid / 5, k = tid - s * 5;
      lds[tid] = sp[s * 6 + (k < 3 ? k : k + 1)];          // b0 b1 b2 . a1 a2
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int k = 0; k < 5; ++k) c[s][k] = lds[s * 5 + k];
    __syncthreads();                                       // lds becomes st after pass 1
  }

  double z[S][2];
  double sy = 0.0, sx = 0.0;

  // ---- pass 1: zero-state end state per chunk; columns of A^Lc
#pragma unroll
  for (int s = 0; s < S; ++s) {
    z[s][0] = (hj == 2 * s) ? 1.0 : 0.0;
    z[s][1] = (hj == 2 * s + 1) ? 1.0 : 0.0;
  }
  eq_run_chunk<S, EQ_STATE>(xr, len, p.Lc, c, z, sy, sx, yr, 1.0);
  if (chunk_lane) {
#pragma unroll
    for (int s = 0; s < S; ++s) { st[tid][2 * s] = z[s][0]; st[tid][2 * s + 1] = z[s][1]; }
  } else if (hj < N) {
#pragma unroll
    for (int s = 0; s < S; ++s) { Mt[hj][2 * s] = z[s][0]; Mt[hj][2 * s + 1] = z[s][1]; }
  }
  __syncthreads();

  // ---- carry: s_{c+1} = A^Lc s_c + f_c over the chunks that have a successor. Wave 0, one matrix row per lane; lanes >= N
  // shadow row N-1 and write nothing (v_readlane needs the source lanes active, which lanes 0 .. N-1 are).
  if (tid < 64 && p.nfull > 0) {
    const int i = tid < N ? tid : N - 1;
    double row[N];
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = Mt[j][i];
    double sv = 0.0;
    double f = st[0][i];
    for (int cc = 0; cc < p.nfull; ++cc) {
      const double fn = (cc + 1 < p.nfull) ? st[cc + 1][i] : 0.0;      // next chunk's f: off the dependent path
      double a0 = f, a1 = 0.0;
#pragma unroll
      for (int j = 0; j < N; j += 2) {
        a0 += row[j] * eq_bcast(sv, j);
        a1 += row[j + 1] * eq_bcast(sv, j + 1);
      }
      sv = a0 + a1;
      if (tid < N) st[cc][i] = sv;
      f = fn;
    }
  }
  __syncthreads();

  // ---- pass 2 (and 3): the chunk from its true start state
  const bool has_prev = chunk_lane && tid > 0 && tid <= p.nfull;
  double z0[S][2];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    z0[s][0] = has_prev ? st[tid - 1][2 * s] : 0.0;
    z0[s][1] = has_prev ? st[tid - 1][2 * s + 1] : 0.0;
  }
#pragma unroll
  for (int s = 0; s < S; ++s) { z[s][0] = z0[s][0]; z[s][1] = z0[s][1]; }
  if (!p.match_rms) {
    eq_run_chunk<S, EQ_WRITE>(xr, len, p.Lc, c, z, sy, sx, yr, 1.0);
    return;
  }
  eq_run_chunk<S, EQ_SUMS>(xr, len, p.Lc, c, z, sy, sx, yr, 1.0);
  __syncthreads();                                          // every lane has read its start state: st becomes red
  red[0][tid] = sy; red[1][tid] = sx;
  __syncthreads();
  for (int off = EQ_THREADS / 2; off > 0; off >>= 1) {      // fixed tree: the same bits on every call
    if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
    __syncthreads();
  }
  const double rms_y = sqrt(red[0][0] / (double)p.T), rms_x = sqrt(red[1][0] / (double)p.T);
  const double gain = rms_x / (rms_y + 1e-8);
#pragma unroll
  for (int s = 0; s < S; ++s) { z[s][0] = z0[s][0]; z[s][1] = z0[s][1]; }
  eq_run_chunk<S, EQ_WRITE>(xr, len, p.Lc, c, z, sy, sx, yr, gain);
}

// params2sos (util/contentvec/audio_utils.py:5-173) in float64: one thread per (row, band)
__global__ void peq_sos_kernel(const float* __restrict__ gains_db, const float* __restrict__ q, const double* __restrict__ fc, int n_bands,
                               double fs, long total, double* __restrict__ sos) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int band = (int)(idx % n_bands);
  const double G = (double)gains_db[idx], Q = (double)q[idx];
  const double g = pow(10.0, G / 20.0);
  const double A = fmax(0.0, sqrt(g));
  const double w = (2.0 * 3.141592653589793 * fmax(fc[band], 2.0)) / fs;
  const double co = cos(w), si = sin(w);
  double b0, b1, b2, a0, a1, a2;
  if (band != 0 && band != n_bands - 1) {                  // peaking
    const double alpha = si / (Q * 2.0);
    const double c2 = -2.0 * co;
    b0 = 1.0 + alpha * A; b1 = c2; b2 = 1.0 - alpha * A;
    a0 = 1.0 + alpha / A; a1 = c2; a2 = 1.0 - alpha / A;
  } else {
    const double am = A - 1.0, ap = A + 1.0;
    const double beta = si * sqrt(A) / Q;
    const double amc = am * co;
    if (band == 0) {                                       // low shelf
      b0 = A * (ap - amc + beta); b1 = A * 2.0 * (am - ap * co); b2 = A * (ap - amc - beta);
      a0 = ap + amc + beta; a1 = -2.0 * (am + ap * co); a2 = ap + amc - beta;
    } else {                                               // high shelf
      b0 = A * (ap + amc + beta); b1 = A * -2.0 * (am + ap * co); b2 = A * (ap + amc - beta);
      a0 = ap - amc + beta; a1 = 2.0 * (am - ap * co); a2 = ap - amc - beta;
    }
  }
  double* o = sos + idx * 6;
  o[0] = b0 / a0; o[1] = b1 / a0; o[2] = b2 / a0; o[3] = 1.0; o[4] = a1 / a0; o[5] = a2 / a0;
}

template <int S>
static void launch_sos(const SosP& p, int B, hipStream_t stream) {
  hipLaunchKernelGGL(sos_filter_kernel<S>, dim3(B), dim3(EQ_THREADS), 0, stream, p);
}

}  // namespace tdvc

extern "C" size_t tdvc_sos_filter_workspace(int32_t B, int32_t T, int32_t n_sections) {
  (void)B; (void)T; (void)n_sections;
  return 0;                                                // the chunk states live in LDS; the RMS pass recomputes instead of storing
}

extern "C" int tdvc_sos_filter(const float* x, int64_t x_bs, const double* sos, int32_t B, int32_t T, int32_t n_sections, int32_t match_rms,
                               float* y, int64_t y_bs, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  (void)workspace; (void)workspace_bytes;
  if (B < 0) return tdvc_fail(TDVC_EINVAL, "sos_filter: negative batch");
  if (T < 0) return tdvc_fail(TDVC_EUNSUPPORTED, "sos_filter: T must be >= 1");
  if (n_sections < 1 || n_sections > EQ_MAX_S) return tdvc_fail(TDVC_EUNSUPPORTED, "sos_filter: needs 1 <= n_sections <= 16");
  if (B == 0 || T == 0) return TDVC_OK;
  if (!x || !sos || !y) return tdvc_fail(TDVC_EINVAL, "sos_filter: null pointer");
  if (x_bs < 0 || y_bs < 0 || (B > 1 && y_bs < T)) return tdvc_fail(TDVC_EINVAL, "sos_filter: bad row stride (output rows must not overlap)");
  SosP p;
  p.x = x; p.x_bs = x_bs; p.sos = sos; p.T = T;
  p.Lc = (int)(((long)T + EQ_CHUNKS - 1) / EQ_CHUNKS);
  p.nfull = (int)(((long)T + p.Lc - 1) / p.Lc) - 1;        // <= EQ_CHUNKS - 1
  p.match_rms = match_rms ? 1 : 0;
  p.y = y; p.y_bs = y_bs;
  hipStream_t st = (hipStream_t)stream;
  switch (n_sections) {
#define EQ_CASE(S) case S: launch_sos<S>(p, B, st); break;
    EQ_CASE(1) EQ_CASE(2) EQ_CASE(3) EQ_CASE(4) EQ_CASE(5) EQ_CASE(6) EQ_CASE(7) EQ_CASE(8)
    EQ_CASE(9) EQ_CASE(10) EQ_CASE(11) EQ_CASE(12) EQ_CASE(13) EQ_CASE(14) EQ_CASE(15) EQ_CASE(16)
#undef EQ_CASE
  }
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_peq_sos(const float* gains_db, const float* q, const double* fc, int32_t n_bands, double sample_rate, int32_t B,
                            double* sos, void* stream) {
  using namespace tdvc;
  if (n_bands < 2) return tdvc_fail(TDVC_EINVAL, "peq_sos: needs n_bands >= 2 (a low and a high shelf)");
  if (B < 0 || !(sample_rate > 0.0)) return tdvc_fail(TDVC_EINVAL, "peq_sos: bad batch or sample rate");
  if (B == 0) return TDVC_OK;
  if (!gains_db || !q || !fc || !sos) return tdvc_fail(TDVC_EINVAL, "peq_sos: null pointer");
  const long total = (long)B * n_bands;
  hipLaunchKernelGGL(peq_sos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     gains_db, q, fc, n_bands, sample_rate, total, sos);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
