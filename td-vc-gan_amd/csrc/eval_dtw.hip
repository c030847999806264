// Exact dynamic time warping of a batch of sequence pairs: the alignment step of the reference's objective evaluation
// (test_scripts/common/test_mcd.py: fastdtw(test_mcep, ref_mcep, dist=2), reported as dist / len(path)), without fastdtw's radius.
//
// tdvc_dtw: one block per pair, BH threads. The programme is cut into bands of BH rows; a band is swept along its anti-diagonals,
// thread l owning row r0 + l with its x_i in registers and working on column j = k - l at step k:
//   refill    every 64 steps the block stages the next 64 rows of y into an LDS ring of BH + 64 columns and the next 64 cells of the
//             band's upper boundary row. A ring row is DT floats, D padded with zeros to the instance's DT = 4, 16, 28 or 64 (x_i
//             likewise), so that the distance loop is straight-line code; the row stride DT | 1 is odd, so the 64 lanes of a
//             wave, which read 64 consecutive columns, hit different banks
//   exchange  up = C(i-1, j) is what the neighbour lane held after the previous step: a cross-lane move inside a wave, one LDS
//             slot per wave across waves (double-buffered); diag = C(i-1, j-1) is the `up` of the previous step, left = the
//             lane's own previous cell. Lane 0 of the band reads the boundary row from LDS.
//   cell      d(i, j) in fp32 from direct differences, C = d + the FIRST minimum of (up, left, diag) in float64, len = len(pred) + 1
//   store     the last row of a band goes to the workspace as the next band's boundary (in place: column j is read at step <= j
//             and written at step j + BH - 1); with a path, 2-bit directions, 16 columns per 32-bit word and row
//   barrier   ONE per step
// After the last band thread 0 walks the directions back from (n-1, m-1) and writes the path from its start (the length is known
// from the carried count), all threads pad the rest with -1. No atomics, no allocation, a fixed evaluation order.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"

namespace tdvc {

constexpr int DTW_MAX_LEN = 4096;
constexpr int DTW_MAX_D = 64;
constexpr int DTW_CH = 64;                                  // columns per refill
constexpr int DTW_MAX_WAVES = 16;
constexpr size_t DTW_FIXED_LDS = 1280;                      // wave slots [2][16], boundary stage [64] (float64 + int32 each), the length: 1172 B
constexpr size_t DTW_LDS_BUDGET = 160 * 1024;

struct DtwP {
  const float* x; long x_bs, x_fs;
  const float* y; long y_bs, y_fs;
  const int* nlen; const int* mlen;
  int N, M, D, metric;
  double* cost; int* length;
  int* path; long path_bs;
  double* bnd_c; int* bnd_l;                               // [B][M] boundary row between bands
  unsigned* dirs; long dirs_bs; int dirs_rs;               // [B][N][ceil(M / 16)] directions, NULL without a path
};

static inline int dtw_dir_words(int M) { return (M + 15) / 16; }
static inline size_t dtw_bnd_c_bytes(int B, int M) { return tdvc_align256((size_t)B * M * sizeof(double)); }
static inline size_t dtw_bnd_l_bytes(int B, int M) { return tdvc_align256((size_t)B * M * sizeof(int)); }
static constexpr size_t dtw_lds_bytes(int DT, int BH) { return DTW_FIXED_LDS + (size_t)(BH + DTW_CH) * (DT | 1) * sizeof(float); }

template <int DT, int BH>
__global__ __launch_bounds__(BH) void dtw_kernel(DtwP p) {
  extern __shared__ __attribute__((aligned(16))) double dtw_lds[];            // all of it dynamic: a kernel with static LDS cannot raise its cap to 160 KB
  double (*s_slot_c)[DTW_MAX_WAVES] = reinterpret_cast<double (*)[DTW_MAX_WAVES]>(dtw_lds);                 // [2][16]
  double* s_bnd_c = dtw_lds + 2 * DTW_MAX_WAVES;                                                               // [64]
  int (*s_slot_l)[DTW_MAX_WAVES] = reinterpret_cast<int (*)[DTW_MAX_WAVES]>(s_bnd_c + DTW_CH);              // [2][16]
  int* s_bnd_l = reinterpret_cast<int*>(s_bnd_c + DTW_CH) + 2 * DTW_MAX_WAVES;                                 // [64]
  int& s_len = s_bnd_l[DTW_CH];
  float* dtw_ring = reinterpret_cast<float*>(dtw_lds) + DTW_FIXED_LDS / sizeof(float);
  constexpr int RC = BH + DTW_CH;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long b = blockIdx.x;
  constexpr int Dp = DT | 1;                               // ring row: DT floats (zeros from D on), odd stride
  const int D = p.D, metric = p.metric;
  int n = p.nlen ? p.nlen[b] : p.N;
  int m = p.mlen ? p.mlen[b] : p.M;
  n = n < 0 ? 0 : (n > p.N ? p.N : n);                     // the lengths live on the device: clamped, never trusted
  m = m < 0 ? 0 : (m > p.M ? p.M : m);
  if (n == 0 || m == 0) {                                  // block-uniform
    if (t == 0) { p.cost[b] = (double)NAN; p.length[b] = 0; }
    return;
  }
  const float* xb = p.x + b * p.x_bs;
  const float* yb = p.y + b * p.y_bs;
  double* bnd_c = p.bnd_c + b * p.M;
  int* bnd_l = p.bnd_l + b * p.M;
  unsigned* dirs = p.dirs ? p.dirs + b * p.dirs_bs : nullptr;
  const double INF = (double)INFINITY;

  for (int r0 = 0; r0 < n; r0 += BH) {
    const int rows = n - r0 < BH ? n - r0 : BH;
    const int i = r0 + t;
    const bool mine = t < rows;
    const bool first_band = r0 == 0, write_bnd = r0 + BH < n;
    float xr[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) xr[d] = (mine && d < D) ? xb[(long)i * p.x_fs + d] : 0.f;
    double cur_c = INF, diag_c = INF;                      // my last cell (the next cell's left); the previous step's up
    int cur_l = 0, diag_l = 0;
    unsigned word = 0;
    int slot = 0;                                          // ring slot of my column, j mod RC
    const int steps = m + rows - 1;
    for (int k = 0; k < steps; ++k) {
      if ((k & (DTW_CH - 1)) == 0) {
        // columns [k, k + 64) take the slots of columns [k - RC, k - RC + 64), which no lane reads after step k - 1
        const int cn = m - k < DTW_CH ? m - k : DTW_CH;
        const int s0 = k % RC;
        for (int idx = t; idx < cn * DT; idx += BH) {
          const int c = idx / DT, d = idx - c * DT;
          int s = s0 + c;
          s = s >= RC ? s - RC : s;
          dtw_ring[s * Dp + d] = d < D ? yb[(long)(k + c) * p.y_fs + d] : 0.f;
        }
        if (!first_band && t < cn) { s_bnd_c[t] = bnd_c[k + t]; s_bnd_l[t] = bnd_l[k + t]; }
        __syncthreads();
      }
      const int j = k - t;
      double up_c = __shfl_up(cur_c, 1);
      int up_l = __shfl_up(cur_l, 1);
      if (lane == 0) {
        if (w > 0) { up_c = s_slot_c[(k + 1) & 1][w - 1]; up_l = s_slot_l[(k + 1) & 1][w - 1]; }
        else if (first_band) { up_c = INF; up_l = 0; }
        else { up_c = s_bnd_c[k & (DTW_CH - 1)]; up_l = s_bnd_l[k & (DTW_CH - 1)]; }      // thread 0: j == k
      }
      if (mine && j >= 0 && j < m) {
        const float* yr = dtw_ring + slot * Dp;
        float s = 0.f;
        if (metric == TDVC_DTW_L1) {
#pragma unroll
          for (int d = 0; d < DT; ++d) s += fabsf(xr[d] - yr[d]);                // x and y are both 0 from D on: exact zeros, no branch
        } else {
#pragma unroll
          for (int d = 0; d < DT; ++d) { const float e = xr[d] - yr[d]; s = fmaf(e, e, s); }
          if (metric == TDVC_DTW_L2) s = __fsqrt_rn(s);
        }
        const double left_c = j == 0 ? INF : cur_c;
        const double dg_c = j == 0 ? INF : diag_c;
        double best = up_c; int bl = up_l; unsigned dir = 0;             // the first minimum in the order up, left, diagonal
        if (left_c < best) { best = left_c; bl = cur_l; dir = 1; }
        if (dg_c < best) { best = dg_c; bl = diag_l; dir = 2; }
        if (i == 0 && j == 0) { best = 0.0; bl = 0; }
        diag_c = up_c; diag_l = up_l;
        cur_c = (double)s + best; cur_l = bl + 1;
        if (dirs) {
          word |= dir << (2 * (j & 15));
          if ((j & 15) == 15 || j == m - 1) { dirs[(long)i * p.dirs_rs + (j >> 4)] = word; word = 0; }
        }
        if (write_bnd && t == BH - 1) { bnd_c[j] = cur_c; bnd_l[j] = cur_l; }
        if (i == n - 1 && j == m - 1) { p.cost[b] = cur_c; p.length[b] = cur_l; s_len = cur_l; }
        slot = slot + 1 == RC ? 0 : slot + 1;
      }
      if (lane == 63) { s_slot_c[k & 1][w] = cur_c; s_slot_l[k & 1][w] = cur_l; }
      __syncthreads();
    }
  }

  if (p.path) {                                            // the last step's barrier made s_len and every direction word visible
    int* out = p.path + b * p.path_bs;
    const int len = s_len, cap = p.N + p.M - 1;
    for (int q = len + t; q < cap; q += BH) { out[2 * q] = -1; out[2 * q + 1] = -1; }
    if (t == 0) {
      int i = n - 1, j = m - 1;
      unsigned wd = dirs[(long)i * p.dirs_rs + (j >> 4)];
      for (int q = len - 1; q >= 0; --q) {                 // len cells whatever the words hold: the walk cannot run away
        out[2 * q] = i; out[2 * q + 1] = j;
        const unsigned dir = (wd >> (2 * (j & 15))) & 3u;
        int ni = i - (dir != 1u), nj = j - (dir != 0u);
        ni = ni < 0 ? 0 : ni; nj = nj < 0 ? 0 : nj;
        if (ni != i || (nj >> 4) != (j >> 4)) wd = dirs[(long)ni * p.dirs_rs + (nj >> 4)];
        i = ni; j = nj;
      }
    }
  }
}

template <int DT, int BH>
static void launch_dtw(const DtwP& p, int B, hipStream_t st) {
  const size_t lds = dtw_lds_bytes(DT, BH);
  if (lds > 64 * 1024) TDVC_BIG_LDS_ONCE((dtw_kernel<DT, BH>));
  TDVC_TRACE((dtw_kernel<DT, BH>));
  hipLaunchKernelGGL((dtw_kernel<DT, BH>), dim3(B), dim3(BH), lds, st, p);
}

}  // namespace tdvc

extern "C" size_t tdvc_dtw_workspace(int32_t B, int32_t N, int32_t M, int32_t want_path) {
  using namespace tdvc;
  if (B < 1 || N < 1 || M < 1 || N > DTW_MAX_LEN || M > DTW_MAX_LEN) return 0;
  return dtw_bnd_c_bytes(B, M) + dtw_bnd_l_bytes(B, M) + (want_path ? (size_t)B * N * dtw_dir_words(M) * sizeof(unsigned) : 0);
}

extern "C" int tdvc_dtw(const float* x, int64_t x_bs, int64_t x_fs, const float* y, int64_t y_bs, int64_t y_fs, const int32_t* n,
                        const int32_t* m, int32_t B, int32_t N, int32_t M, int32_t D, int32_t metric, double* cost, int32_t* length,
                        int32_t* path, int64_t path_bs, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0) return tdvc_fail(TDVC_EINVAL, "dtw: negative batch");
  if (N < 1 || M < 1 || D < 1) return tdvc_fail(TDVC_EINVAL, "dtw: N, M and D must be positive");
  if (metric != TDVC_DTW_L2 && metric != TDVC_DTW_L1 && metric != TDVC_DTW_SQ)
    return tdvc_fail(TDVC_EINVAL, "dtw: unknown metric (TDVC_DTW_L2, TDVC_DTW_L1 or TDVC_DTW_SQ)");
  if (x_fs < D || y_fs < D || x_bs < 0 || y_bs < 0)
    return tdvc_fail(TDVC_EINVAL, "dtw: bad stride (frames are D dense values, batch strides are not negative)");
  if (path && (path_bs < 0 || (B > 1 && path_bs < 2 * ((int64_t)N + M - 1))))
    return tdvc_fail(TDVC_EINVAL, "dtw: path rows of 2 * (N + M - 1) values must not overlap");
  if (N > DTW_MAX_LEN || M > DTW_MAX_LEN || D > DTW_MAX_D) return tdvc_fail(TDVC_EUNSUPPORTED, "dtw: needs N, M <= 4096 and D <= 64");
  if (B == 0) return TDVC_OK;
  if (!x || !y || !cost || !length) return tdvc_fail(TDVC_EINVAL, "dtw: null pointer");
  if (!workspace || workspace_bytes < tdvc_dtw_workspace(B, N, M, path != nullptr))
    return tdvc_fail(TDVC_EWORKSPACE, "dtw: workspace is null or smaller than tdvc_dtw_workspace");
  DtwP p;
  p.x = x; p.x_bs = x_bs; p.x_fs = x_fs; p.y = y; p.y_bs = y_bs; p.y_fs = y_fs; p.nlen = n; p.mlen = m;
  p.N = N; p.M = M; p.D = D; p.metric = metric; p.cost = cost; p.length = length; p.path = path; p.path_bs = path_bs;
  char* ws = (char*)workspace;
  p.bnd_c = (double*)ws;
  p.bnd_l = (int*)(ws + dtw_bnd_c_bytes(B, M));
  p.dirs = path ? (unsigned*)(ws + dtw_bnd_c_bytes(B, M) + dtw_bnd_l_bytes(B, M)) : nullptr;
  p.dirs_rs = dtw_dir_words(M);
  p.dirs_bs = (long)N * p.dirs_rs;
  hipStream_t st = (hipStream_t)stream;
  // D is padded with zeros to the next of 4, 16, 28, 64 (mel-cepstra of order 24 are D = 25, or 24 without c0), so that the distance
  // loop is DT straight-line steps; the band is the widest whose ring fits: 1024 rows up to 28, 512 above
  if (D <= 4) launch_dtw<4, 1024>(p, B, st);
  else if (D <= 16) launch_dtw<16, 1024>(p, B, st);
  else if (D <= 28) launch_dtw<28, 1024>(p, B, st);
  else launch_dtw<64, 512>(p, B, st);
  static_assert(dtw_lds_bytes(28, 1024) <= DTW_LDS_BUDGET && dtw_lds_bytes(64, 512) <= DTW_LDS_BUDGET, "ring over the LDS budget");
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
