// YIN pitch tracker (util/yin.py:24-140): waveform in, one F0 value per frame out, in ONE launch.
//
// One 256-thread block per (sample, frame). The frame u[0..L), L = 2*tau_max <= 2048 floats, is staged into LDS with the
// reference's zero padding done by index arithmetic. The difference function
//     d[tau] = sum_{j=0}^{L-1-tau} (u[j] - u[j+tau])^2
// is summed directly (the reference's FFT form E + S[L-tau] - S[tau] - 2*corr cancels badly at the minimum). A thread owns
// four consecutive tau (tau0 = 4g) and a slice of j; it walks j four at a time with a sliding register window over
// u[j+tau0 .. j+tau0+7), so two ds_read_b128 (u[j..j+3], the same address in every lane of a slice = broadcast, and the next
// four window values, consecutive 16-byte slots over consecutive lanes = conflict-free) feed 16 subtract-FMA pairs. Rows have
// L - tau terms, so the j range of a row is cut into NC slices of equal length PER ROW: every thread gets the same share of
// its own row, and with several blocks resident per CU the 2:1 spread between the first and the last row evens out.
// Built with -fno-slp-vectorize (csrc/Makefile): packed into v_pk_add/v_pk_fma the loop needs 94 instead of 52 VGPRs and ran 20 % slower.
//
// Accuracy: the test bound is a few fp32 ulps of the CMDF, less than a plain running sum of 2048 terms keeps. Sums run in
// blocks of 16 terms that are folded into the row total with a compensated (Kahan) add: fp32 throughout, +4 VALU per 32.
// Every sum has a fixed order (no atomics): two runs give identical bits.
//
// After the difference function everything stays in LDS: slice fold, prefix sum (4 values per thread, wave64 shuffle scan,
// one cross-wave step), CMDF, and the two searches as block min / sum reductions.
#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"
#include "pitch_yin.h"

namespace tdvc {

struct YinP {
  const float* x; long x_bs;
  int T, tau_min, tau_max, stride, n_frames;
  int NG, NC;                                     // groups of YIN_R tau; j slices per row
  float threshold, sample_rate; int soft;
  float* f0; float* cmdf;
};

// The phases live in pitch_yin.h (the soft-YIN backward recomputes them with the same code).
__global__ __launch_bounds__(YIN_THREADS) void yin_f0_kernel(YinP p) {
  __shared__ __attribute__((aligned(16))) float u[YIN_U_FLOATS];
  __shared__ __attribute__((aligned(16))) float dpart[YIN_D_FLOATS];
  __shared__ float redf[YIN_RED_SLOTS * YIN_WAVES];
  __shared__ int redi[2 * YIN_WAVES];

  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.n_frames, f = blockIdx.x - b * p.n_frames;
  const int L = 2 * p.tau_max;

  yin_stage_frame(p.x, p.x_bs, p.T, p.tau_max, p.stride, b, f, u);
  __syncthreads();
  yin_difference(u, dpart, L, p.NG, p.NC);
  __syncthreads();

  const int n = p.tau_max - 1 - p.tau_min;
  float* cl = u;                                                // the frame is dead: its LDS holds the CMDF from here on
  {
    float d[4], S[4];
    yin_cmdf(dpart, redf, cl, p.tau_min, p.tau_max, p.NG, p.NC, d, S);
  }
  __syncthreads();

  const long fr = (long)b * p.n_frames + f;
  if (p.cmdf) {
    float* out = p.cmdf + fr * n;
    for (int k = tid; k < n; k += YIN_THREADS) out[k] = cl[k];
  }

  float tau;
  if (!p.soft) {
    // first index below the threshold (index 0 counts as none), then the first index from there on whose successor is not smaller
    int fb = INT_MAX;
    for (int k = tid; k < n; k += YIN_THREADS)
      if (cl[k] < p.threshold) { fb = k; break; }
    fb = yin_block_min(fb, redi, 0);
    int cand = INT_MAX;
    if (fb != INT_MAX && fb > 0) {
      for (int k = tid; k < n; k += YIN_THREADS)
        if (k >= fb && (k == n - 1 || cl[k + 1] - cl[k] >= 0.f)) { cand = k; break; }
    }
    cand = yin_block_min(cand, redi, 1);
    tau = (cand == INT_MAX) ? 0.f : (float)cand;
  } else {
    // tau = sum_k softmax(-100 c)[k] * k, times 1 if any c is below the threshold
    float mn, se, sk;
    yin_soft_search(cl, n, redf, mn, se, sk);
    tau = (mn < p.threshold) ? sk / se : 0.f;
  }
  if (tid == 0) p.f0[fr] = yin_f0_of_tau(tau, p.tau_min, p.sample_rate);
}

}  // namespace tdvc

extern "C" int tdvc_yin_num_frames(int32_t T, int32_t tau_max, int32_t stride) {
  if (T < 1 || tau_max < 1 || stride < 1) return 0;
  const long L = 2L * tau_max;
  return (int)(((T > L ? (long)T : L) - 1) / stride + 1);
}

extern "C" int tdvc_yin_f0(const float* x, int64_t x_bs, int32_t B, int32_t T, int32_t tau_min, int32_t tau_max, int32_t stride,
                           float threshold, int32_t soft, float sample_rate, float* f0, float* cmdf, void* stream) {
  using namespace tdvc;
  if (T < 1) return tdvc_fail(TDVC_EINVAL, "yin_f0: T must be >= 1");
  if (stride < 1) return tdvc_fail(TDVC_EINVAL, "yin_f0: stride must be >= 1");
  if (tau_min < 0 || (long)tau_max - 1 - tau_min < 2) return tdvc_fail(TDVC_EINVAL, "yin_f0: needs 0 <= tau_min and tau_max - 1 - tau_min >= 2");
  if (tau_max > YIN_TAU_CAP) return tdvc_fail(TDVC_EUNSUPPORTED, "yin_f0: tau_max above 1024 (the frame no longer fits the kernel's LDS image)");
  if (B < 1 || x_bs < 0 || !(sample_rate > 0.f)) return tdvc_fail(TDVC_EINVAL, "yin_f0: bad batch, batch stride or sample rate");
  if (!x || !f0) return tdvc_fail(TDVC_EINVAL, "yin_f0: null pointer");
  const int nf = tdvc_yin_num_frames(T, tau_max, stride);
  if ((long)B * nf > INT_MAX) return tdvc_fail(TDVC_EUNSUPPORTED, "yin_f0: more than 2^31-1 frames in one call");
  YinP p;
  p.x = x; p.x_bs = x_bs; p.T = T; p.tau_min = tau_min; p.tau_max = tau_max; p.stride = stride; p.n_frames = nf;
  p.NG = (tau_max + YIN_R - 1) / YIN_R;
  p.NC = YIN_THREADS / p.NG;                                   // NG <= 256, so NC >= 1 and NC * NG <= 256
  p.threshold = threshold; p.sample_rate = sample_rate; p.soft = soft ? 1 : 0;
  p.f0 = f0; p.cmdf = cmdf;
  auto k = yin_f0_kernel;
  TDVC_TRACE(k);
  hipLaunchKernelGGL(k, dim3(B * nf), dim3(YIN_THREADS), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
