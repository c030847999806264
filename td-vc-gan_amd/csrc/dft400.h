// The 400-point DFT stage of the two mel front ends (voice_mel_kernel in eval_speaker.hip, fbank_db_kernel in eval_ecapa.hip): 25 ms
// frames at 16 kHz, a hop of 10 ms, 8 frames per block. The host hands both kernels one float64 table (_host.dft_tables)
//     cos[400] | sin[400] | window[400] | filterbank[n_mels][201],      cos/sin at the angle 2 pi m / 400.
// Each kernel stages its own windowed samples into xw (padding and gain differ) and runs its own mel loop over pw.
#pragma once
#include <hip/hip_runtime.h>

namespace tdvc {

constexpr int DFT_NFFT = 400, DFT_HOP = 160, DFT_BINS = 201;
constexpr int DFT_FR = 8;                                   // frames per block
constexpr int DFT_TAB_WINDOW = 2 * DFT_NFFT, DFT_TAB_FB = 3 * DFT_NFFT;

// LDS of a block, declared by the kernel as three arrays (as members of one struct xw lost its 16-byte alignment and ds_read_b128):
//     double cs[2 * DFT_NFFT]        the table's cos | sin, copied by the kernel
//     double xw[DFT_FR][DFT_NFFT]    windowed samples of the block's frames
//     double pw[DFT_FR][DFT_BINS]    their power spectra
// pw = |DFT(xw)|^2 by direct summation in float64, samples in ascending order; bin k reads the table at k i mod 400, walked as
// m += k without a division. The caller puts a barrier between its stores to xw / cs and this, and one behind it.
template <int THREADS>
__device__ __forceinline__ void dft400_power(const double* cs, const double (*xw)[DFT_NFFT], double (*pw)[DFT_BINS], int t) {
  for (int item = t; item < DFT_FR * DFT_BINS; item += THREADS) {
    const int fr = item / DFT_BINS, k = item - fr * DFT_BINS;
    double re = 0.0, im = 0.0;
    int m = 0;
    for (int i = 0; i < DFT_NFFT; ++i) {
      const double v = xw[fr][i];
      re = fma(v, cs[m], re);
      im = fma(v, cs[DFT_NFFT + m], im);
      m += k;
      if (m >= DFT_NFFT) m -= DFT_NFFT;
    }
    pw[fr][k] = re * re + im * im;
  }
}

}  // namespace tdvc
