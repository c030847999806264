// Device code shared by the stride-1 weight-gradient kernels (conv_wgrad_lean.hip, conv_wgrad_pipe.hip): what a wave does
// with operand tiles once they are staged. A wave owns M_REP x C_REP sub-tiles of 16 (co) x 16 (ci) for all J taps; lane
// (ln = lane & 15, kq = lane >> 4) holds column ln and rows 4*kq .. 4*kq+3 of each. Staging, loop shape and pipeline
// interleave differ per kernel and stay with the kernels.
//
// Only helpers that leave every kernel's machine code as it was live here. The accumulator clear, the 2x2-wave slab store
// (tile, pipe) and the bias row partial (lean, tile) were tried as helpers too, each in several spellings; every one moved
// the compiler's schedule in the kernels that would share it, so those kernels keep their own copies.
#pragma once
#include "conv_wgrad_lean.h"

namespace tdvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The A / B fragments of one k-step (4 time steps): A = dy' (row co = ln, k = kq), B = x' (k = kq, column ci = ln).
// a_lane / x_lane point at the lane's element of step 0 in LDS tiles with row strides AS / XS; tap j reads x' j*D to the
// right, so every address is base + immediate. The kernels keep two fragment sets (av[2][M_REP], bv[2][C_REP][J]) and load
// step s+1 before the MFMAs of step s issue.
template <int AS, int XS, int D, int M_REP, int C_REP, int J>
__device__ __forceinline__ void wg_frag_load(float (&av)[M_REP], float (&bv)[C_REP][J], const float* a_lane, const float* x_lane, int nn) {
#pragma unroll
  for (int m = 0; m < M_REP; ++m) av[m] = a_lane[nn + m * 16 * AS];
#pragma unroll
  for (int c = 0; c < C_REP; ++c)
#pragma unroll
    for (int j = 0; j < J; ++j) bv[c][j] = x_lane[nn + c * 16 * XS + j * D];
}

// D[co][ci] += dy'[co][t] * x'[t + j*D][ci]
template <int M_REP, int C_REP, int J>
__device__ __forceinline__ void wg_frag_mma(const float (&av)[M_REP], const float (&bv)[C_REP][J], f32x4 (&acc)[M_REP][C_REP][J]) {
#pragma unroll
  for (int m = 0; m < M_REP; ++m)
#pragma unroll
    for (int c = 0; c < C_REP; ++c)
#pragma unroll
      for (int j = 0; j < J; ++j)
        acc[m][c][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[c][j], acc[m][c][j], 0, 0, 0);
}

// Bias partials of a block whose row sums went 16 lanes per row (lean, tile): the lane with (tid & 15) == 0 holds rows
// (tid >> 4) + 16*i of the tile in bias_part[i] and writes them behind the weights of the block's slab.
template <int NB>
__device__ __forceinline__ void wg_bias_store(const float (&bias_part)[NB], const WgLeanP& p, float* slab, int r0, int tid) {
  if ((tid & 15) == 0) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int row = r0 + (tid >> 4) + 16 * i;
      if (row < p.R) slab[p.bias_off + row] = bias_part[i];
    }
  }
}

}  // namespace tdvc
