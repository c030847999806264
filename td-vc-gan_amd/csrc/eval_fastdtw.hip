// FastDTW (Salvador & Chan, in the form of the `fastdtw` Python package) of a batch of sequence pairs: the alignment the reference's
// objective evaluation calls (test_scripts/common/test_mcd.py: fastdtw(test_mcep, ref_mcep, dist=2), reported as dist / len(path)).
// The definition is written out in include/tdvc.h; tests/fastdtw_ref.py restates it literally in float64.
//
// tdvc_fastdtw: ONE launch, one block of 256 threads per pair, the whole pyramid inside it:
//   levels     n_0 = n, n_{l+1} = n_l / 2 (m likewise) while both are >= radius + 2; level l + 1 is fp32(0.5f * (a + b)) of level l,
//              built by all threads into the workspace (level 0 is the caller's array, read through its strides)
//   window     the coarsest level is solved in full; every other level inside the window of the coarser path, by the closed form
//              of include/tdvc.h: row i covers columns [lo(i), hi(i)], both non-decreasing in i
//   recurrence along ANTI-DIAGONALS k = i + j. A diagonal crosses at most 4 r + 2 rows of a window (derivation at FD_CW below), so
//              one wave holds a diagonal with room to spare: lane l owns the rows i = l (mod 64), of which at most one is live, and
//              keeps its last cell in registers. up = C(i-1, j) is the neighbour lane's last cell (a rotation of the wave), diag =
//              C(i-1, j-1) is the `up` of the previous step, left the lane's own last cell; a lane whose row has no cell on the
//              diagonal carries +inf, which is exactly "outside the window". C = d + the FIRST minimum of (up, left, diag) in
//              float64, the length is carried with it. The serial chain is n_l + m_l - 1 steps per level, with no barrier.
//   distances  do not depend on the recurrence, so waves 1..3 run ahead of it: a tile is 64 diagonals; while wave 0 sweeps tile t
//              from one LDS buffer, the other waves fill the second buffer with the fp32 distances of tile t + 1 (the (4 r + 2)
//              candidate rows from the first live row of each diagonal, +inf where the row has no cell there). One barrier per tile.
//   directions 2 bits per (diagonal, lane), gathered with two ballots: 16 bytes per diagonal, whatever the radius
//   back-trace wave 0 walks the directions from (n_l - 1, m_l - 1) on the scalar unit, 64 diagonals in its lanes at a time and the
//              next 64 in flight, and leaves the first and last column of the path in every row (the next window), or at level
//              0 the path itself
// No atomics, no allocation, no host synchronisation, a fixed evaluation order: graph-capturable and bit-identical from call to call.
// Every index that comes out of the workspace (bounds, first live rows, directions) is clamped or range-checked before it is used
// as an address, so the kernel stays inside its buffers whatever the workspace held.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "conv_common.h"

namespace tdvc {

constexpr int FD_MAX_LEN = 16384;
constexpr int FD_MAX_D = 64;
constexpr int FD_MAX_R = 8;
constexpr int FD_NT = 256;                                  // wave 0: the recurrence; waves 1..3: the distances of the next tile
constexpr int FD_TILE = 64;                                 // anti-diagonals per tile
// Rows on one anti-diagonal. Let rows i1 < i2 both have a cell on diagonal k: k - i1 <= hi(i1) and k - i2 >= lo(i2), so
// i2 - i1 <= hi(i1) - lo(i2). With c = i / 2, a1 = min(c1 + r, n_c - 1), a2 = max(c2 - r, 0): hi(i1) <= 2 (jmax(a1) + r) + 1 and
// lo(i2) >= 2 (jmin(a2) - r). If a2 > a1 the path is monotone, jmin(a2) >= jmax(a1), and i2 - i1 <= 4 r + 1. Otherwise
// c2 - r <= a2 <= a1 <= c1 + r, so c2 - c1 <= 2 r and again i2 - i1 <= 4 r + 1. A diagonal therefore crosses at most 4 r + 2 rows,
// and a window has at most (4 r + 2) (n + m - 1) cells. The unwindowed coarsest level has min(n, m) <= r + 1 rows or columns.
constexpr int FD_CW = 4 * FD_MAX_R + 2;
constexpr int FD_CWP = FD_CW + 2;
constexpr int FD_MAX_LEVELS = 16;                           // 16384 -> 2 is 14 levels

struct FdtwP {
  const float* x; long x_bs, x_fs;
  const float* y; long y_bs, y_fs;
  const int* nlen; const int* mlen;
  int N, M, D, metric, radius;
  double* cost; int* length;
  int* path; long path_bs;
  float* xpyr; float* ypyr;                                 // [B][N D], [B][M D]: levels 1.. of each pair, dense, one after another
  int* lo; int* hi; int* jmin; int* jmax;                   // [B][N] each: the window of the current level, the path's columns per row
  int* ifirst;                                              // [B][N + M]: first live row of every anti-diagonal of the current level
  ulonglong2* dirs;                                         // [B][N + M]: direction bit 0 / bit 1 of the 64 lanes of every anti-diagonal
};

// Workspace of one call, an upper bound by construction:
//   pyramids    sum_{l >= 1} floor(n / 2^l) <= n - 1 < N frames of D floats per side
//   window      lo, hi and the path's first / last column: one int32 per row of a level, n_l <= N
//   diagonals   n_l + m_l - 1 < N + M per level; the first live row (int32) and the directions of each. A diagonal has at most
//               4 r + 2 <= 34 cells (above) and 64 direction slots of 2 bits, so the (4 r + 2) (n + m - 1) cells of a window fit
//               in 16 (N + M) bytes for every radius up to 8
// Levels are solved one after another, so one set of per-level buffers serves them all.
struct FdtwWs { size_t xpyr, ypyr, lo, hi, jmin, jmax, ifirst, dirs, total; };
static inline FdtwWs fd_workspace(int B, int N, int M, int D) {
  FdtwWs w;
  size_t o = 0;
  w.xpyr = o; o += tdvc_align256((size_t)B * N * D * sizeof(float));
  w.ypyr = o; o += tdvc_align256((size_t)B * M * D * sizeof(float));
  w.lo = o; o += tdvc_align256((size_t)B * N * sizeof(int));
  w.hi = o; o += tdvc_align256((size_t)B * N * sizeof(int));
  w.jmin = o; o += tdvc_align256((size_t)B * N * sizeof(int));
  w.jmax = o; o += tdvc_align256((size_t)B * N * sizeof(int));
  w.ifirst = o; o += tdvc_align256((size_t)B * ((size_t)N + M) * sizeof(int));
  w.dirs = o; o += tdvc_align256((size_t)B * ((size_t)N + M) * sizeof(ulonglong2));
  w.total = o;
  return w;
}

__device__ __forceinline__ float fd_dist(const float* a, const float* b, int D, int metric) {
  float s = 0.f;                                            // tdvc_dtw's distances: direct differences, summed in order of d
  const bool l1 = metric == TDVC_DTW_L1;
  int d0 = 0;
  for (; d0 + 8 <= D; d0 += 8) {                            // 16 loads in flight, then their 8 terms: a loop of one load pair per
    float av[8], bv[8];                                     // term waits out a memory latency for every element
#pragma unroll
    for (int u = 0; u < 8; ++u) { av[u] = a[d0 + u]; bv[u] = b[d0 + u]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) { const float e = av[u] - bv[u]; s = l1 ? s + fabsf(e) : fmaf(e, e, s); }
  }
  if (d0 < D) {                                             // the last D mod 8 terms the same way; an absent term is an exact zero
    float av[7], bv[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) { const bool in = d0 + u < D; av[u] = in ? a[d0 + u] : 0.f; bv[u] = in ? b[d0 + u] : 0.f; }
#pragma unroll
    for (int u = 0; u < 7; ++u) { const float e = av[u] - bv[u]; s = l1 ? s + fabsf(e) : fmaf(e, e, s); }
  }
  return metric == TDVC_DTW_L2 ? __fsqrt_rn(s) : s;
}

// The value of the lane below, lane 0 from lane 63: a rotation of the whole wave by one lane in the data path (DPP wave_ror:1),
// not a trip through the LDS crossbar, because this move is on the chain of the recurrence.
__device__ __forceinline__ int fd_from_lane_below(int v) { return __builtin_amdgcn_mov_dpp(v, 0x13C, 0xF, 0xF, true); }
__device__ __forceinline__ double fd_from_lane_below(double v) {
  return __hiloint2double(fd_from_lane_below(__double2hiint(v)), fd_from_lane_below(__double2loint(v)));
}

__device__ __forceinline__ int fd_clamp(int v, int a, int b) { return v < a ? a : (v > b ? b : v); }

__global__ __launch_bounds__(FD_NT) void fastdtw_kernel(FdtwP p) {
  __shared__ float s_d[2][FD_TILE][FD_CWP];                 // 18 KB: the distances of two tiles
  __shared__ int s_if[2][FD_TILE];
  __shared__ int s_n[FD_MAX_LEVELS], s_m[FD_MAX_LEVELS];
  __shared__ long s_xo[FD_MAX_LEVELS], s_yo[FD_MAX_LEVELS];
  __shared__ int s_levels, s_len;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long b = blockIdx.x;
  const int D = p.D, metric = p.metric, r = p.radius, cw = 4 * r + 2;
  int n = p.nlen ? p.nlen[b] : p.N;
  int m = p.mlen ? p.mlen[b] : p.M;
  n = fd_clamp(n, 0, p.N);                                  // the lengths live on the device: clamped, never trusted
  m = fd_clamp(m, 0, p.M);
  const int cap = p.N + p.M - 1;
  int* out = p.path ? p.path + b * p.path_bs : nullptr;
  if (n == 0 || m == 0) {                                   // block-uniform
    if (t == 0) { p.cost[b] = (double)NAN; p.length[b] = 0; }
    if (out) for (int q = t; q < cap; q += FD_NT) { out[2 * q] = -1; out[2 * q + 1] = -1; }
    return;
  }
  float* xpyr = p.xpyr + b * (long)p.N * D;
  float* ypyr = p.ypyr + b * (long)p.M * D;
  int* lo = p.lo + b * p.N;
  int* hi = p.hi + b * p.N;
  int* jmin = p.jmin + b * p.N;
  int* jmax = p.jmax + b * p.N;
  int* ifirst = p.ifirst + b * ((long)p.N + p.M);
  ulonglong2* dirs = p.dirs + b * ((long)p.N + p.M);
  const double INF = (double)INFINITY;

  if (t == 0) {                                             // the level sizes, from the pair's own lengths
    int nl = n, ml = m, L = 0;
    long xo = 0, yo = 0;
    s_n[0] = nl; s_m[0] = ml; s_xo[0] = 0; s_yo[0] = 0;
    while (nl >= r + 2 && ml >= r + 2 && L + 1 < FD_MAX_LEVELS) {
      nl >>= 1; ml >>= 1; ++L;
      s_n[L] = nl; s_m[L] = ml; s_xo[L] = xo; s_yo[L] = yo;
      xo += (long)nl * D; yo += (long)ml * D;
    }
    s_levels = L + 1;
  }
  __syncthreads();
  const int levels = s_levels;
  const float* x0 = p.x + b * p.x_bs;
  const float* y0 = p.y + b * p.y_bs;

  for (int l = 1; l < levels; ++l) {                        // the fp32 pyramid: one rounding of a + b per level, the halving is exact
    for (int side = 0; side < 2; ++side) {
      const float* src = side ? (l == 1 ? y0 : ypyr + s_yo[l - 1]) : (l == 1 ? x0 : xpyr + s_xo[l - 1]);
      const long ss = l == 1 ? (side ? p.y_fs : p.x_fs) : D;
      float* dst = side ? ypyr + s_yo[l] : xpyr + s_xo[l];
      const int cnt = (side ? s_m[l] : s_n[l]) * D;
      for (int base = t; base < cnt; base += 4 * FD_NT) {   // four pairs of loads in flight per thread, then their four stores
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = base + u * FD_NT, i = idx / D, d = idx - i * D;
          const bool in = idx < cnt;
          av[u] = in ? src[(long)(2 * i) * ss + d] : 0.f;
          bv[u] = in ? src[(long)(2 * i + 1) * ss + d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (base + u * FD_NT < cnt) dst[base + u * FD_NT] = 0.5f * (av[u] + bv[u]);
      }
    }
    __syncthreads();
  }

  for (int lev = levels - 1; lev >= 0; --lev) {
    const int nl = s_n[lev], ml = s_m[lev], K = nl + ml - 1;
    const float* xl = lev ? xpyr + s_xo[lev] : x0;
    const float* yl = lev ? ypyr + s_yo[lev] : y0;
    const long xs = lev ? D : p.x_fs, ys = lev ? D : p.y_fs;
    const bool want_dirs = lev > 0 || out != nullptr;

    // the window of this level, from the coarser path's first / last column per row (closed form, include/tdvc.h)
    if (lev == levels - 1) {
      for (int i = t; i < nl; i += FD_NT) { lo[i] = 0; hi[i] = ml - 1; }
    } else {
      const int nc = s_n[lev + 1];
      for (int i = t; i < nl; i += FD_NT) {
        const int ci = i >> 1;                              // n_c for an odd last row: only the radius covers it
        const int first = jmin[fd_clamp(ci - r, 0, nc - 1)], last = jmax[fd_clamp(ci + r, 0, nc - 1)];
        lo[i] = fd_clamp(2 * (fd_clamp(first, 0, ml) - r), 0, ml - 1);
        hi[i] = fd_clamp(2 * (fd_clamp(last, 0, ml) + r) + 1, 0, ml - 1);
      }
    }
    if (t == 0) s_len = 0;
    __syncthreads();
    // first live row of diagonal k = min { i : hi(i) + i >= k }; hi(i) + i increases strictly, so row i owns a run of k
    for (int i = t; i < nl; i += FD_NT) {
      const int k1 = hi[i] + i;
      for (int k = i ? hi[i - 1] + i : 0; k <= k1; ++k) ifirst[k] = i;
    }
    __syncthreads();

    auto produce = [&](int tile, int buf, int tid, int nthreads) {
      const int k0 = tile * FD_TILE;
      for (int idx = tid; idx < FD_TILE * cw; idx += nthreads) {
        const int kk = idx / cw, c = idx - kk * cw, k = k0 + kk;
        if (k >= K) break;
        const int f = ifirst[k];
        if (c == 0) s_if[buf][kk] = f;
        const int row = f + c, j = k - row;
        float d = INFINITY;                                 // no cell: an infinite distance, so the cell's cost is +inf by itself
        if (row >= 0 && row < nl && j >= lo[row] && j <= hi[row]) d = fd_dist(xl + (long)row * xs, yl + (long)j * ys, D, metric);
        s_d[buf][kk][c] = d;
      }
    };
    produce(0, 0, t, FD_NT);
    __syncthreads();

    // my last cell (the next cell's left) and the previous step's up (the diagonal), each with its length. Every cell starts at
    // +inf, except that lane 0 sees a diagonal predecessor of cost 0 and length 0 at step 0: that makes C(0, 0) = d(0, 0)
    double c1 = INF, pu = lane == 0 ? 0.0 : INF;
    int l1 = 0, pul = 0;
    const int ntiles = (K + FD_TILE - 1) / FD_TILE;
    for (int tile = 0; tile < ntiles; ++tile) {
      const int buf = tile & 1;
      if (w == 0) {
        const int k0 = tile * FD_TILE, steps = K - k0 < FD_TILE ? K - k0 : FD_TILE;
        const int fv = s_if[buf][lane];                     // lane kk holds the first live row of diagonal k0 + kk (unused past `steps`)
        auto fetch = [&](int kk) {                          // my distance on diagonal k0 + kk, +inf without a cell there
          const int c = (lane - __builtin_amdgcn_readlane(fv, kk)) & 63;
          return c < cw ? s_d[buf][kk][c] : INFINITY;
        };
        float d1 = fetch(0), d2 = steps > 1 ? fetch(1) : INFINITY;
        for (int kk = 0; kk < steps; ++kk) {
          const float d = d1;
          d1 = d2;
          if (kk + 2 < steps) d2 = fetch(kk + 2);           // LDS reads two steps ahead: none is on the chain of the recurrence
          const double up = fd_from_lane_below(c1);         // lane l - 1, lane 0 from lane 63: rows i - 1 and i are neighbours mod 64
          const int upl = fd_from_lane_below(l1);
          double best = up; int bl = upl; unsigned dir = 0;             // the first minimum in the order up, left, diagonal
          if (c1 < best) { best = c1; bl = l1; dir = 1; }
          if (pu < best) { best = pu; bl = pul; dir = 2; }
          pu = up; pul = upl;
          c1 = (double)d + best;
          l1 = bl + 1;
          if (want_dirs) {
            const unsigned long long b0 = __ballot(dir & 1u), b1 = __ballot(dir >> 1);
            if (lane == 0) dirs[k0 + kk] = make_ulonglong2(b0, b1);
          }
        }
        if (tile == ntiles - 1 && lane == ((nl - 1) & 63)) {            // after the last diagonal this lane holds cell (n_l - 1, m_l - 1)
          s_len = l1;
          if (lev == 0) { p.cost[b] = c1; p.length[b] = l1; }
        }
      } else if (tile + 1 < ntiles) {
        produce(tile + 1, buf ^ 1, t - 64, FD_NT - 64);
      }
      __syncthreads();
    }

    if (want_dirs) {                                        // the barrier above made s_len and every direction word visible
      const int len = s_len < K ? s_len : K;
      if (lev == 0) for (int q = len + t; q < cap; q += FD_NT) { out[2 * q] = -1; out[2 * q + 1] = -1; }
      if (w == 0) {
        // The walk is one chain of dependent steps, so it runs on the scalar unit: the cell (i, j) is wave-uniform, lane l holds
        // the words of diagonal 64 c + l of the current chunk c, and a step is a lane read with a scalar index. The chunk below
        // is loaded while the current one is walked (a step goes down one or two diagonals, so chunks are visited in order).
        auto load = [&](int c) {
          const int k = c * 64 + lane;
          return (c >= 0 && k < K) ? dirs[k] : make_ulonglong2(0ull, 0ull);
        };
        int i = __builtin_amdgcn_readfirstlane(nl - 1), j = __builtin_amdgcn_readfirstlane(ml - 1);
        int q = __builtin_amdgcn_readfirstlane(len - 1), pi = -1;
        ulonglong2 nxt = load((i + j) >> 6);
        for (int c = (i + j) >> 6; q >= 0; --c) {           // one chunk per round; len cells whatever the words hold: no running away
          int x0 = (int)(unsigned)nxt.x, x1 = (int)(unsigned)(nxt.x >> 32), y0 = (int)(unsigned)nxt.y, y1 = (int)(unsigned)(nxt.y >> 32);
          // the chunk's words are waited for HERE, once, and before the next chunk's load is issued: left to their first use, the
          // wait lands inside the loop below, where it would also wait, at every step, for the stores of the step before
          asm volatile("" : "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1));
          nxt = load(c - 1);
          while (q >= 0 && ((i + j) >> 6) == c) {
            if (lane == 0) {
              if (lev == 0) { out[2 * q] = i; out[2 * q + 1] = j; }
              else { if (i != pi) jmax[i] = j; jmin[i] = j; }
            }
            pi = i;
            const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((i & 32) ? x1 : x0, (i + j) & 63);
            const unsigned b1 = (unsigned)__builtin_amdgcn_readlane((i & 32) ? y1 : y0, (i + j) & 63);
            const unsigned dir = ((b0 >> (i & 31)) & 1u) | (((b1 >> (i & 31)) & 1u) << 1);
            int ni = i - (dir != 1u), nj = j - (dir != 0u);
            ni = ni < 0 ? 0 : ni; nj = nj < 0 ? 0 : nj;
            if (ni == i && nj == j) q = 0;                  // (0, 0) reached (or a stuck word): nothing is left to walk
            i = ni; j = nj; --q;
          }
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace tdvc

extern "C" size_t tdvc_fastdtw_workspace(int32_t B, int32_t N, int32_t M, int32_t D, int32_t radius, int32_t want_path) {
  using namespace tdvc;
  (void)want_path;                                          // the coarser levels need their directions with or without a path
  if (B < 1 || N < 1 || M < 1 || D < 1 || N > FD_MAX_LEN || M > FD_MAX_LEN || D > FD_MAX_D || radius < 1 || radius > FD_MAX_R) return 0;
  return fd_workspace(B, N, M, D).total;
}

extern "C" int tdvc_fastdtw(const float* x, int64_t x_bs, int64_t x_fs, const float* y, int64_t y_bs, int64_t y_fs, const int32_t* n,
                            const int32_t* m, int32_t B, int32_t N, int32_t M, int32_t D, int32_t metric, int32_t radius, double* cost,
                            int32_t* length, int32_t* path, int64_t path_bs, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace tdvc;
  if (B < 0) return tdvc_fail(TDVC_EINVAL, "fastdtw: negative batch");
  if (N < 1 || M < 1 || D < 1) return tdvc_fail(TDVC_EINVAL, "fastdtw: N, M and D must be positive");
  if (metric != TDVC_DTW_L2 && metric != TDVC_DTW_L1 && metric != TDVC_DTW_SQ)
    return tdvc_fail(TDVC_EINVAL, "fastdtw: unknown metric (TDVC_DTW_L2, TDVC_DTW_L1 or TDVC_DTW_SQ)");
  if (radius < 1) return tdvc_fail(TDVC_EINVAL, "fastdtw: the radius must be at least 1 (only the radius covers an odd last row)");
  if (x_fs < D || y_fs < D || x_bs < 0 || y_bs < 0)
    return tdvc_fail(TDVC_EINVAL, "fastdtw: bad stride (frames are D dense values, batch strides are not negative)");
  if (path && path_bs < 2 * ((int64_t)N + M - 1)) return tdvc_fail(TDVC_EINVAL, "fastdtw: path rows hold 2 * (N + M - 1) values");
  if (N > FD_MAX_LEN || M > FD_MAX_LEN || D > FD_MAX_D || radius > FD_MAX_R)
    return tdvc_fail(TDVC_EUNSUPPORTED, "fastdtw: needs N, M <= 16384, D <= 64 and radius <= 8");
  if (B == 0) return TDVC_OK;
  if (!x || !y || !cost || !length) return tdvc_fail(TDVC_EINVAL, "fastdtw: null pointer");
  if (!workspace || workspace_bytes < tdvc_fastdtw_workspace(B, N, M, D, radius, path != nullptr))
    return tdvc_fail(TDVC_EWORKSPACE, "fastdtw: workspace is null or smaller than tdvc_fastdtw_workspace");
  const FdtwWs o = fd_workspace(B, N, M, D);
  char* ws = (char*)workspace;
  FdtwP p;
  p.x = x; p.x_bs = x_bs; p.x_fs = x_fs; p.y = y; p.y_bs = y_bs; p.y_fs = y_fs; p.nlen = n; p.mlen = m;
  p.N = N; p.M = M; p.D = D; p.metric = metric; p.radius = radius; p.cost = cost; p.length = length; p.path = path; p.path_bs = path_bs;
  p.xpyr = (float*)(ws + o.xpyr); p.ypyr = (float*)(ws + o.ypyr);
  p.lo = (int*)(ws + o.lo); p.hi = (int*)(ws + o.hi); p.jmin = (int*)(ws + o.jmin); p.jmax = (int*)(ws + o.jmax);
  p.ifirst = (int*)(ws + o.ifirst); p.dirs = (ulonglong2*)(ws + o.dirs);
  hipStream_t st = (hipStream_t)stream;
  TDVC_TRACE(fastdtw_kernel);
  hipLaunchKernelGGL(fastdtw_kernel, dim3(B), dim3(FD_NT), 0, st, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
