// Banded max-sum (Viterbi) decoder over a per-frame salience lattice: the temporal decoding step of the reference's inference
// pitch tracker (util.crepe.filtered_pitch(signal, "viterbi") -> torchcrepe decode.viterbi), generic in the lattice, the band and the
// prior, so that the CMDF of tdvc_yin_f0 and a caller's own activations go through the same launch.
//
// tdvc_viterbi_path: one block per row, frames serial, states across lanes. P = 1, 2 or 4 lanes share one destination state j
// (P the largest with n * P <= 1024) and split its W predecessors k = q, q + P, q + 2P, ... between them, so the speech lattice
// (n = 233, W = 64) runs 16 dependent LDS steps per frame instead of 64. Per frame:
//   scan      lane (j, q): best of u[lo[j] + k] + t[j][k] over its k, strict > in ascending k (lowest predecessor on a tie)
//   combine   the P lanes of a state by shuffles: larger value, then lower predecessor
//   floor     against (-jump, a), a = the previous frame's first argmax: with the scores renormalised to max 0 that is the best
//             out-of-band candidate, and the clamp max(logw, -jump) is folded into the table when it is staged
//   store     u_f[j] = obs[f][j] + best to the other LDS buffer, the predecessor as uint16 to the workspace
//   reduce    block max and first argmax of u_f (wave shuffles, one LDS slot per wave, ONE barrier per frame)
// u is the unnormalised score of the frame; the next frame subtracts max(u_f) from `best`, which is the renormalisation
// d_f = u_f - max(u_f) without a second barrier. Scores stay bounded for any F. A state whose every candidate is -inf points to
// predecessor 0, which is what the tie rule gives over all n candidates.
// The table is staged once as t[k / P][thread] (lane-contiguous, conflict-free): in LDS when it fits beside the two score
// buffers, else in the row's slice of the workspace, which the same block reads back through the cache, coalesced. The next frame's
// lattice row is loaded a frame ahead. After the last frame thread 0 walks the predecessors back: F dependent loads that hit the
// L2 (the table of 1120 x 233 predecessors is 0.5 MB). No atomics, no allocation, a fixed evaluation order.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"

namespace tdvc {

constexpr int VT_MAX_N = 1024;
constexpr int VT_MAX_W = 256;
constexpr int VT_MAX_THREADS = 1024;
constexpr int VT_PAD = 4;                                  // score-buffer slots past n that the padded k of the last states read
constexpr int VT_RED = 2 * 2 * (VT_MAX_THREADS / 64);       // reduction slots: value and index per wave, double-buffered
constexpr size_t VT_LDS_BYTES = 160 * 1024;               // all of it dynamic: the kernel declares no static LDS
constexpr int VT_NO_PRED = 0x7fffffff;

struct VitP {
  const float* x; long x_bs, x_fs;
  float scale; const float* prior;
  const float* logw; const int* lo; int W;
  float jump;
  int F, n, M;                                             // M = ceil(W / P) scan steps
  int* path; long path_bs;
  unsigned short* bp;                                      // [B][F][n] predecessors (frame 0 unused)
  float* tab_ws; long tab_ws_bs;                           // the staged table per row when it does not fit the LDS
};

static inline int vt_parts(int n) { return n * 4 <= VT_MAX_THREADS ? 4 : n * 2 <= VT_MAX_THREADS ? 2 : 1; }
static inline int vt_threads(int n) { return (n * vt_parts(n) + 63) / 64 * 64; }
static inline size_t vt_fixed_lds(int n) { return (size_t)(2 * (n + VT_PAD) + VT_RED) * sizeof(float); }
static inline size_t vt_tab_bytes(int n, int W) {
  const int P = vt_parts(n);
  return (size_t)((W + P - 1) / P) * vt_threads(n) * sizeof(float);
}

// larger value wins, the lower index on a tie
__device__ __forceinline__ void vt_better(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// Block max and first argmax of (v, i) over the lanes that hold a state; the others pass (-inf, VT_NO_PRED). One barrier.
__device__ __forceinline__ void vt_block_argmax(float v, int i, float* redv, int* redi, int nw, float& m, int& a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float v2 = __shfl_xor(v, off);
    const int i2 = __shfl_xor(i, off);
    vt_better(v, i, v2, i2);
  }
  if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = i; }
  __syncthreads();
  m = redv[0]; a = redi[0];
  for (int w = 1; w < nw; ++w) vt_better(m, a, redv[w], redi[w]);
}

template <int P, bool TAB_LDS>
__global__ __launch_bounds__(VT_MAX_THREADS) void viterbi_kernel(VitP p) {
  extern __shared__ __attribute__((aligned(16))) float vt_lds[];
  const int n = p.n, W = p.W, M = p.M, F = p.F;
  const int NT = blockDim.x, nw = NT >> 6;
  const int t = threadIdx.x;
  const long b = blockIdx.x;
  const int ustride = n + VT_PAD;                          // two score buffers, the reduction slots, then the table
  float* redv = vt_lds + 2 * ustride;                      // [2][16]
  int* redi = reinterpret_cast<int*>(redv + VT_RED / 2);   // [2][16]
  float* tab;
  if constexpr (TAB_LDS) tab = vt_lds + 2 * ustride + VT_RED; else tab = p.tab_ws + b * p.tab_ws_bs;

  const bool live = t < n * P;                             // lanes past the last state shadow it and store nothing
  const int j = live ? t / P : n - 1;
  const int q = t % P;
  const bool owner = live && q == 0;
  int lo_j = p.lo[j];
  lo_j = lo_j < 0 ? 0 : (lo_j > n - W ? n - W : lo_j);     // a band is kept inside [0, n) whatever the table says: no stray read
  const float pr = p.prior ? p.prior[j] : 0.f;
  const float nj = -p.jump;

  // ---- stage the table: t[m][thread] = max(logw[j][m*P + q], -jump), -inf in the slots past W and in the shadow lanes
  for (int idx = t; idx < M * NT; idx += NT) {
    const int tt = idx % NT, k = (idx / NT) * P + tt % P;
    if (tt >= n * P || k >= W) tab[idx] = -INFINITY;
  }
  for (int s = t; s < n * W; s += NT) {                    // source order: coalesced reads, scattered writes, once
    const int sj = s / W, k = s - sj * W;
    tab[(k / P) * NT + sj * P + k % P] = fmaxf(p.logw[s], nj);
  }
  if (t < VT_PAD) { vt_lds[n + t] = 0.f; vt_lds[ustride + n + t] = 0.f; }

  // ---- frame 0
  const float* xr = p.x + b * p.x_bs + j;
  float xv = xr[0];
  float xn = F > 1 ? xr[p.x_fs] : 0.f;
  float u = fmaf(p.scale, xv, pr);
  if (owner) vt_lds[j] = u;
  float m; int a;
  vt_block_argmax(owner ? u : -INFINITY, owner ? j : VT_NO_PRED, redv, redi, nw, m, a);

  unsigned short* bp = p.bp + (size_t)b * F * n;
  const float* tp = tab + t;
  for (int f = 1; f < F; ++f) {
    const float* up = vt_lds + ((f - 1) & 1) * ustride + lo_j + q;
    xv = xn;
    if (f + 1 < F) xn = xr[(long)(f + 1) * p.x_fs];        // a frame ahead of its use
    float bv = -INFINITY;
    int bm = 0;
#pragma unroll 8
    for (int mm = 0; mm < M; ++mm) {
      const float v = up[mm * P] + tp[(size_t)mm * NT];
      if (v > bv) { bv = v; bm = mm; }
    }
    int bi = q < W ? lo_j + q + bm * P : VT_NO_PRED;       // a lane with no slot of the band never wins a tie
#pragma unroll
    for (int off = 1; off < P; off <<= 1) {
      const float v2 = __shfl_xor(bv, off);
      const int i2 = __shfl_xor(bi, off);
      vt_better(bv, bi, v2, i2);
    }
    bv -= (m > -INFINITY) ? m : 0.f;                       // renormalise: the previous frame's maximum becomes 0
    vt_better(bv, bi, nj, a);                              // the uniform floor, through the previous frame's first argmax
    if (bv == -INFINITY) bi = 0;                           // every one of the n candidates is -inf
    u = fmaf(p.scale, xv, pr) + bv;
    if (owner) {
      vt_lds[(f & 1) * ustride + j] = u;
      bp[(size_t)f * n + j] = (unsigned short)bi;
    }
    vt_block_argmax(owner ? u : -INFINITY, owner ? j : VT_NO_PRED, redv + (f & 1) * (VT_MAX_THREADS / 64), redi + (f & 1) * (VT_MAX_THREADS / 64), nw, m, a);
  }

  // ---- trace back from the first argmax of the last frame
  __syncthreads();                                         // the predecessors of every wave are visible to thread 0
  if (t == 0) {
    int* out = p.path + b * p.path_bs;
    int s = a;
    out[F - 1] = s;
    for (int f = F - 1; f > 0; --f) {
      s = bp[(size_t)f * n + s];
      out[f - 1] = s;
    }
  }
}

template <int P>
static void launch_viterbi(const VitP& p, int B, int threads, bool tab_lds, size_t lds, hipStream_t st) {
  if (tab_lds) {
    if (lds > 64 * 1024) TDVC_BIG_LDS_ONCE((viterbi_kernel<P, true>));
    hipLaunchKernelGGL((viterbi_kernel<P, true>), dim3(B), dim3(threads), lds, st, p);
  } else {
    hipLaunchKernelGGL((viterbi_kernel<P, false>), dim3(B), dim3(threads), lds, st, p);
  }
}

// workspace layout: predecessors [B][F][n] uint16, then (n large enough that some W <= 256 does not fit the LDS) B table slices
static inline size_t vt_bp_bytes(int B, int F, int n) { return tdvc_align256((size_t)B * F * n * sizeof(unsigned short)); }
static inline size_t vt_tab_slice(int n) {
  const size_t worst = vt_tab_bytes(n, VT_MAX_W);
  return vt_fixed_lds(n) + worst > VT_LDS_BYTES ? tdvc_align256(worst) : 0;
}

}  // namespace tdvc

extern "C" size_t tdvc_viterbi_workspace(int32_t B, int32_t F, int32_t n) {
  using namespace tdvc;
  if (B < 1 || F < 1 || n < 1 || n > VT_MAX_N) return 0;
  return vt_bp_bytes(B, F, n) + (size_t)B * vt_tab_slice(n);
}

extern "C" int tdvc_viterbi_path(const float* x, int64_t x_bs, int64_t x_fs, float scale, const float* prior, const float* logw,
                                 const int32_t* lo, int32_t W, float jump, int32_t B, int32_t F, int32_t n, int32_t* path,
                                 int64_t path_bs, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0) return tdvc_fail(TDVC_EINVAL, "viterbi_path: negative batch");
  if (n < 1 || F < 1 || W < 1) return tdvc_fail(TDVC_EINVAL, "viterbi_path: n, F and W must be positive");
  if (W > n) return tdvc_fail(TDVC_EINVAL, "viterbi_path: a band of W > n predecessors leaves [0, n)");
  if (!(jump >= 0.f)) return tdvc_fail(TDVC_EINVAL, "viterbi_path: jump must be >= 0 (+inf disables the floor)");
  if (x_fs < n || x_bs < 0 || path_bs < 0 || (B > 1 && path_bs < F))
    return tdvc_fail(TDVC_EINVAL, "viterbi_path: bad stride (lattice rows are n dense values, path rows must not overlap)");
  if (n > VT_MAX_N || W > VT_MAX_W) return tdvc_fail(TDVC_EUNSUPPORTED, "viterbi_path: needs n <= 1024 and W <= 256");
  if (B == 0) return TDVC_OK;
  if (!x || !logw || !lo || !path) return tdvc_fail(TDVC_EINVAL, "viterbi_path: null pointer");
  if (!workspace || workspace_bytes < tdvc_viterbi_workspace(B, F, n))
    return tdvc_fail(TDVC_EWORKSPACE, "viterbi_path: workspace is null or smaller than tdvc_viterbi_workspace");
  const int P = vt_parts(n);
  VitP p;
  p.x = x; p.x_bs = x_bs; p.x_fs = x_fs; p.scale = scale; p.prior = prior; p.logw = logw; p.lo = lo; p.W = W; p.jump = jump;
  p.F = F; p.n = n; p.M = (W + P - 1) / P; p.path = path; p.path_bs = path_bs;
  p.bp = (unsigned short*)workspace;
  p.tab_ws = (float*)((char*)workspace + vt_bp_bytes(B, F, n));
  p.tab_ws_bs = (long)(vt_tab_slice(n) / sizeof(float));
  const bool tab_lds = vt_fixed_lds(n) + vt_tab_bytes(n, W) <= VT_LDS_BYTES;
  const size_t lds = vt_fixed_lds(n) + (tab_lds ? vt_tab_bytes(n, W) : 0);
  hipStream_t st = (hipStream_t)stream;
  switch (P) {
    case 4: launch_viterbi<4>(p, B, vt_threads(n), tab_lds, lds, st); break;
    case 2: launch_viterbi<2>(p, B, vt_threads(n), tab_lds, lds, st); break;
    default: launch_viterbi<1>(p, B, vt_threads(n), tab_lds, lds, st); break;
  }
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
