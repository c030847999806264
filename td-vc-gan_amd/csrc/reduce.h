// Reductions of the operator kernels (pitch_*, eval_*, ssl_wavlm), one definition each. No atomics: a shuffle butterfly inside a
// wave, then a combine of the per-wave values through LDS, both in a fixed order, so the result is bit-identical from call to call.
// Two summation orders over the per-wave values exist; they differ in floating point and are part of a kernel's contract:
//   sum_pairwise    (r0 + r1) + (r2 + r3), four waves     DIO, StoneMask, CheapTrick, the voice encoder, Fbank
//   sum_in_order    ((r0 + r1) + r2) + ...                YIN forward and soft-YIN backward
// A new kernel picks one and says so; an existing one keeps the one it has. Minimum and maximum are order-free.
// Barriers: a block_* helper contains ONE barrier, between the write of red and the combine. The barrier that protects red against
// its previous or next use belongs to the caller: the helper cannot know which of the two a kernel needs, and adds neither.
#pragma once
#include <hip/hip_runtime.h>

namespace tdvc {

// xor butterfly over the 64 lanes, offsets 32 .. 1: the same tree, and the result, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// the combine alone, of per-wave values STRIDE apart; for a kernel that passes several values through one barrier
template <int STRIDE = 1, typename T>
__device__ __forceinline__ T sum_pairwise(const T* red) {
  return (red[0] + red[STRIDE]) + (red[2 * STRIDE] + red[3 * STRIDE]);
}
template <int NW, typename T>
__device__ __forceinline__ T sum_in_order(const T* red) {
  T r = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r += red[w];
  return r;
}

// Block reductions: v the thread's value, t its index in a block of 64 NW threads, red NW values; the result is in every thread.
// block_stage alone: for a kernel with several values per barrier, one combining thread, or a barrier before the write.
template <typename T>
__device__ __forceinline__ void block_stage(T wave_value, T* red, int t) {
  if ((t & 63) == 0) red[t >> 6] = wave_value;
  __syncthreads();
}
template <typename T>
__device__ __forceinline__ T block_sum_pairwise(T v, T* red, int t) {
  block_stage(wave_sum(v), red, t);
  return sum_pairwise(red);
}
template <int NW, typename T>
__device__ __forceinline__ T block_sum_in_order(T v, T* red, int t) {
  block_stage(wave_sum(v), red, t);
  return sum_in_order<NW>(red);
}
template <int NW, typename T>
__device__ __forceinline__ T block_max(T v, T* red, int t) {
  block_stage(wave_max(v), red, t);
  T r = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = max(r, red[w]);
  return r;
}
template <int NW, typename T>
__device__ __forceinline__ T block_min(T v, T* red, int t) {
  block_stage(wave_min(v), red, t);
  T r = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = min(r, red[w]);
  return r;
}

// a row's length: lengths[b] clamped to [0, T], T without a lengths array (b int or long, as the kernel has it)
template <typename I>
__device__ __forceinline__ int row_len(const int* lengths, I b, int T) { return lengths ? min(max(lengths[b], 0), T) : T; }

}  // namespace tdvc
