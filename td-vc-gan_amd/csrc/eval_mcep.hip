// Mel-cepstrum of a power spectrum: the pysptk.sp2mc(sp, order, alpha) step of the reference's objective evaluation
// (test_scripts/common/test_mcd.py:47). Everything after the logarithm is linear (inverse real FFT, c[0] / 2, SPTK's frequency
// transform), so the host folds it into one float64 matrix (evaluate.sp2mc_matrix) and the device computes
//     mc[b][f][:] = mat[order + 1][nbins] . log(max(P[b][f][:], floor)).
//
// tdvc_sp2mc: one block per frame. The 256 threads take the logarithm of the frame's bins in float64 into LDS; each of the 4 waves
// then owns the coefficients o = wave, wave + 4, ...: lane l sums bins l, l + 64, ... in ascending order, the 64 partials are
// combined by a butterfly of shuffles (a fixed order), lane 0 rounds once to fp32. The matrix (100 KB at the default settings)
// is read through the L2 by every block. No atomics, bit-identical from call to call.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"

namespace tdvc {

constexpr int MC_MAX_BINS = 2049;                          // n_fft <= 4096
constexpr int MC_MAX_ORDER = 255;
constexpr int MC_THREADS = 256;

struct Sp2mcP {
  const float* power; long p_bs, p_fs, p_ns;
  const double* mat;
  int F, nbins, order;
  float floor_;
  float* mc;
};

__global__ __launch_bounds__(MC_THREADS) void sp2mc_kernel(Sp2mcP p) {
  __shared__ double lp[MC_MAX_BINS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long fr = blockIdx.x;
  const long b = fr / p.F, f = fr - b * p.F;
  const float* src = p.power + b * p.p_bs + f * p.p_fs;
  for (int k = t; k < p.nbins; k += MC_THREADS) lp[k] = log((double)fmaxf(src[(long)k * p.p_ns], p.floor_));
  __syncthreads();
  float* out = p.mc + fr * (p.order + 1);
  for (int o = w; o <= p.order; o += MC_THREADS / 64) {
    const double* row = p.mat + (long)o * p.nbins;
    double s = 0.0;
    for (int k = lane; k < p.nbins; k += 64) s = fma(row[k], lp[k], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[o] = (float)s;
  }
}

}  // namespace tdvc

extern "C" int tdvc_sp2mc(const float* power, int64_t p_bs, int64_t p_fs, int64_t p_ns, const double* mat, int32_t B, int32_t F,
                          int32_t nbins, int32_t order, float floor_, float* mc, void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0) return tdvc_fail(TDVC_EINVAL, "sp2mc: negative batch or frame count");
  if (nbins < 2 || order < 0 || order > nbins - 1) return tdvc_fail(TDVC_EINVAL, "sp2mc: needs nbins >= 2 and 0 <= order <= nbins - 1");
  if (!(floor_ > 0.f) || isinf(floor_)) return tdvc_fail(TDVC_EINVAL, "sp2mc: floor must be positive and finite");
  if (p_bs < 0 || p_fs < 0 || p_ns < 0) return tdvc_fail(TDVC_EINVAL, "sp2mc: negative stride");
  if (nbins > MC_MAX_BINS || order > MC_MAX_ORDER) return tdvc_fail(TDVC_EUNSUPPORTED, "sp2mc: needs nbins <= 2049 and order <= 255");
  if ((int64_t)B * F > 0x7fffffff) return tdvc_fail(TDVC_EUNSUPPORTED, "sp2mc: more than 2^31 - 1 frames");
  if (B == 0 || F == 0) return TDVC_OK;
  if (!power || !mat || !mc) return tdvc_fail(TDVC_EINVAL, "sp2mc: null pointer");
  Sp2mcP p;
  p.power = power; p.p_bs = p_bs; p.p_fs = p_fs; p.p_ns = p_ns; p.mat = mat; p.F = F; p.nbins = nbins; p.order = order;
  p.floor_ = floor_; p.mc = mc;
  hipLaunchKernelGGL(sp2mc_kernel, dim3((unsigned)((int64_t)B * F)), dim3(MC_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
