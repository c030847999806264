// Lean MFMA kernel for the hot stride-1 convolutions (dilated trunk convs, 1x1 posconvs, FiLM conditioning
// convs, D layer 5) and their input-gradients: groups == 1, Tout == Tin, T % 4 == 0, Cin % 4 == 0, weights
// with contiguous (c,k) rows (module layout for forward, the pre-transposed copy for input-grad).
//
// Differences from the generic kernel in conv_mfma.hip (which stays the fallback for strided / transposed /
// grouped / odd shapes and for edge cases):
//   * prologue kind and epilogue kind are template parameters -> no per-element switches, ~5x fewer VALU ops;
//   * MFMA operand roles are swapped (A = input tile, B = weights) so that each lane owns 4 CONSECUTIVE time
//     steps of one output channel: the epilogue reads/writes float4 (dwordx4) instead of scalars;
//   * a compact parameter block (fits in SGPRs without spilling);
//   * interior tiles stage through registers one channel chunk ahead of the MFMA loop (T14 split).
#include "conv_common.h"
#include "conv_lean.h"
#include <algorithm>
#include <type_traits>

PROF_DEFINE(tdvc_debug_lean_prof)

namespace tdvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// prologue kinds LXF_* are declared in conv_lean.h (ACT: none or LeakyReLU by slope)
// LXF_COND: the input tile is not loaded but COMPUTED in the block: rows = channels of FiLM's cond_var.0 output
//   cv0[c][t] = sum_{ce,j} W0x[c][ce][j] * exc[ce][t+j-1] + k3[b][c][edge(t)]   (8 excitation channels, 3 taps, K = 24)
// as a small MFMA pre-pass per channel chunk, LeakyReLU'd straight into the LDS tile that cond_var.2 then convolves;
// the 136-channel intermediate is written once (for the backward pass) and never read back by the forward.



template <int XFK>
__device__ __forceinline__ float lean_xform(const LeanP& p, float v, int b, int c, int q) {
  if (XFK == LXF_ACT) { v = fmaxf(v, v * p.slope); }
  else {
    const float* a = p.aux + (long)b * p.aux_bs + (long)c * p.T + q;
    if (XFK == LXF_FILM) { const float h = v * (1.f + a[0]) + a[(long)p.Cin * p.T]; v = fmaxf(h, h * p.slope); }
    else if (XFK == LXF_MASK_LRELU) { v = a[0] > 0.f ? v : v * p.slope; }
    else { v = v * (1.f - a[0] * a[0]); }
  }
  return v * p.in_scale;
}

template <int XFK>
__device__ __forceinline__ float lean_fetch(const LeanP& p, int b, int c, int q) {
  if (p.reflect) { if (q < 0) q = -q; else if (q >= p.T) q = 2 * (p.T - 1) - q; }
  if (q < 0 || q >= p.T) return 0.f;
  return lean_xform<XFK>(p, p.x[(long)b * p.x_bs + (long)c * p.T + q], b, c, q);
}

#ifndef LEAN_OCC_SMALL
#define LEAN_OCC_SMALL 4      // resident blocks per CU asked for the 16-row tiles (A/B knob: make ab EXTRA=-DLEAN_OCC_SMALL=5)
#endif
// Resident blocks per CU the register budget must allow: 2 for the 48/64/144-row x 256/64-column tiles (>= 36 accumulator
// registers), 3 for 32 x 256, 4 for the rest -- including the 64 x 64 tile (16 accumulator registers), whose 1024-block
// grids (D layer 5) then run as ONE round instead of 1.33 rounds of 768 slots.
constexpr int lean_min_blocks(int m_rep, int n_rep, int wm, int xfk) {
  if (m_rep == 1 && n_rep == 4 && wm == 1 && xfk == LXF_ACT) return 5;   // 16 x 256 tile, plain prologue: 5 resident blocks (<= 96 VGPRs) is what the HBM-bound convs run at
  return m_rep * n_rep >= 9 ? 2 : ((m_rep * n_rep >= 8 || (wm == 4 && xfk == LXF_FILM)) ? 3 : LEAN_OCC_SMALL);   // (FiLM prologue on 64 x 64: 12 spills at 4)
}
// Rows (of the wave's M_REP) the epilogue handles per batch: all operand loads of a batch are in flight together, at most 16 float4
// (64 registers) of them -- the FiLM epilogue has four loaded operands per float4, the others at most two.
constexpr int lean_epi_rows(int m_rep, int n_rep, int epi) {
  int r = 16 / (n_rep * (epi == EPI_FILM ? 4 : 2));
  r = r < 1 ? 1 : (r > m_rep ? m_rep : r);
  while (m_rep % r) --r;
  return r;
}
// ... and sub-tiles of a row: all of them, but two on the 16 x 256 tile with the FiLM epilogue, whose 96 registers (5 resident blocks)
// do not hold four float4 with four operands each beside the accumulators (12 bytes of scratch with all four).
constexpr int lean_epi_cols(int m_rep, int n_rep, int wm, int xfk, int epi) {
  return (m_rep == 1 && n_rep == 4 && wm == 1 && xfk == LXF_ACT && epi == EPI_FILM) ? 2 : n_rep;
}
#ifndef LEAN_RING_1
#define LEAN_RING_1 2         // fragment sets in flight on the tiles with one MFMA per step (A/B knob: make ab EXTRA=-DLEAN_RING_1=4)
#endif
#ifndef LEAN_RING_2
#define LEAN_RING_2 2         // ... with two MFMAs per step
#endif
// Depth of the fragment ring of the MFMA loop; 0 = the one-step-ahead loop with its scalar (tap, channel-group) walk. A wave with one
// or two accumulators has 32 / 64 cycles of matrix work per step and one to four such waves share a SIMD: what a step costs there
// is the instructions it issues around the MFMA (the scalar walk with its branches: 165-360 cycles per step measured), more than the
// LDS latency the loop waits for. The ring loop walks one tap at a time, so a step is the reads, two address adds and the MFMAs,
// with the reads issued `depth` steps ahead of their use and each use waiting for its own reads only (counted lgkmcnt). Measured
// on the classes of profiles/r06_a_lean_frag_pipe_ab.txt, depth 2 beats 4 and 8 on both tiles (deeper rings pay more for the
// fill and drain of every tap than they hide). From four MFMAs per step on the one-step-ahead loop stays.
constexpr int lean_ring_depth(int m_rep, int n_rep) { return m_rep * n_rep == 1 ? LEAN_RING_1 : (m_rep * n_rep == 2 ? LEAN_RING_2 : 0); }
// FOLD: short sequences (T = 16 / 32: discriminator layer 5 of the two sub-sampled discriminators) put p.fold = 64 / T SAMPLES
// side by side in one 64-column tile -- segment s of the LDS tile holds sample b0 + s with its own zero-padded halo, sub-tile
// n of the MFMA loop reads from its sample's segment, the epilogue scatters the sub-tiles back to their samples. Without it
// three quarters (T = 16) or half (T = 32) of every tile's matrix work is padding.
template <int M_REP, int N_REP, int WM, int WN, int XFK, int EPI, bool FOLD = false>
__global__ __launch_bounds__(256, lean_min_blocks(M_REP, N_REP, WM, XFK)) void conv_lean_kernel(const LeanP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int MT = 16 * M_REP * WM, NT = 16 * N_REP * WN;
  constexpr int XVP = (M_REP >= 9 || NT <= 64) ? 4 : (MT >= 32 ? 12 : 6);   // max row-walk passes of the prefetched input tile
  constexpr int WVP = MT >= 48 ? 10 : (MT >= 32 ? 6 : 4);   // ... and of the weight tile
  float* xs = smem;
  float* ws = smem + p.xnp * p.xrp * p.XS;
  constexpr int WX = 25;                                  // odd row stride of the staged W0x chunk
  float* es = ws + p.wnp * p.wrp * p.WS;                  // LXF_COND: excitation tile [Cv][ES]
  float* wx = es + p.Cv * p.ES;                           // LXF_COND: W0x chunk [Cc][WX]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int ln = lane & 15, kq = lane >> 4;
  // Block order. The dispatcher deals blocks round-robin over the 8 XCDs (private L2 each), so with the plain
  // (time tile, row tile, sample) order the row tiles that read one input tile, and the time neighbours that share
  // its halo, sit behind eight different L2s. Remap (bijective for any grid size, cdna_hip_programming.md T1): the
  // blocks that share an XCD take one contiguous run of work items, row tile fastest, then time, then sample.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.swz) {
    const int gx = gridDim.x, gy = gridDim.y;
    const int nwg = gx * gy * gridDim.z;
    const int orig = bx + gx * (by + gy * bz);
    const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    by = wg % gy;
    const int t = wg / gy;
    bx = t % gx; bz = t / gx;
  }
  const int n0 = FOLD ? 0 : bx * NT, r0 = by * MT, b = FOLD ? bz * p.fold : bz;     // FOLD: b = first sample of the tile
  const int wcol0 = wn * 16 * N_REP, wrow0 = wm * 16 * M_REP;
  PROF_DECL

  f32x4 acc[M_REP][N_REP];
#pragma unroll
  for (int m = 0; m < M_REP; ++m)
#pragma unroll
    for (int n = 0; n < N_REP; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int q0 = n0 + p.lo;
  const bool vec_ok = p.vec != 0;                      // rows 16-byte aligned -> float4 staging / epilogue
  // Every 16-byte-aligned tile is staged by the row walk, sequence ends included: a float4 column lies either wholly
  // inside [0, T) or wholly outside (q0 % 4 == 0, T % 4 == 0), and outside columns carry an out-of-range offset, so
  // the buffer loads return the zero padding. Reflect padding (forward trunk convs, ACT prologue only) is patched
  // into the halo columns of the two end tiles after the commit.
  // (the row walk only needs dword-aligned rows: sequences with T % 4 != 0 take it too, with the components past the row
  //  end masked at the commit; only the dwordx4 epilogue needs 16-byte aligned rows)
  const bool interior = (XFK != LXF_COND) && (XFK == LXF_ACT || !p.reflect);
  const bool tail = (p.T & 3) != 0;
  const bool end_tile = q0 < 0 || q0 + p.span > p.T;
  const int jc = p.K * p.Cc;
  const float* xrow0 = p.x + (long)b * p.x_bs;
  const float* arow0 = (XFK != LXF_ACT && XFK != LXF_COND) ? p.aux + (long)b * p.aux_bs : nullptr;
  const float* wgrow = p.w + (long)r0 * p.Cw;

  // Row-walk staging (conv_common.h): thread = (row of the pass, float4 column); a pass covers xrp (wrp) whole rows,
  // so the per-element cost is one buffer load, one offset add and one LDS store -- no index arithmetic in the loop.
  // Rows past the tensor end fall outside the descriptor's range and load as zero.
  RowWalk xw = make_walk(tid, p.span >> 2, p.xrp, p.T, p.XS, q0, p.T);
  if (FOLD) {   // float4 column vv of the staged row = column vv % nvs of segment vv / nvs: same LDS offset, another sample's row
    const int nvec = p.span >> 2, nvs = p.seg >> 2;
    const int rsub = (int)(((float)tid + 0.5f) * (1.0f / (float)nvec));
    const int vv = tid - rsub * nvec;
    const int sg = vv / nvs, q = q0 + 4 * (vv - sg * nvs);
    xw.voff = (xw.active && q >= 0 && q < p.T && b + sg < p.Bn) ? (sg * p.x_bs + rsub * p.T + q) * 4 : 0x7f000000;
  }
  // The descriptors span the tile's samples -- the ones that exist: the row walk's passes run past the chunk's rows and count on the
  // descriptor's end to turn those loads into zeros, so a range reaching over absent samples of the last group let the rows behind
  // the last sample's channels be read from behind the tensor.
  const int fold_bytes = FOLD ? (min(p.fold, p.Bn - b) - 1) * p.x_bs * 4 : 0;
  const RowWalk ww = make_walk(tid, jc >> 2, p.wrp, p.Cw, p.WS, 0, 1 << 30);
  RegTile<XVP> xr;
  RegTile<WVP> wr;
  const bool xpipe = (XFK == LXF_ACT) && interior;
  if (XFK == LXF_COND) {   // excitation tile: positions q0-1 .. q0+span, zero outside the sequence ('same' zero padding)
    const float* eb = p.x + (long)b * p.x_bs;
    for (int r = wave; r < p.Cv; r += 4)
      for (int i = lane; i < p.span + 2; i += 64) {
        const int pos = q0 - 1 + i;
        es[r * p.ES + i] = (pos >= 0 && pos < p.T) ? eb[(long)r * p.T + pos] : 0.f;
      }
  }
  auto x_issue = [&](int c0) {
    const srd_t rs = make_srd(xrow0 + (long)c0 * p.T, (p.Cin - c0) * p.T * 4 + fold_bytes);
    walk_issue<XVP>(xr, rs, xw, p.xnp);
  };
  auto w_issue = [&](int c0) {
    const srd_t rs = make_srd(wgrow + (long)c0 * p.K, ((p.Cout - r0) * p.Cw - c0 * p.K) * 4);
    walk_issue<WVP>(wr, rs, ww, p.wnp);
  };
  if (xpipe) x_issue(0);
  w_issue(0);

  bool needL = false, needR = false;
  if (p.mirror > 0) {
    const int c_lo = n0 + wcol0, c_hi = c_lo + 16 * N_REP - 1;
    needL = (c_lo <= p.mirror) && (c_hi >= 1);
    needR = (c_lo <= p.T - 2) && (c_hi >= p.T - 1 - p.mirror);
  }

  for (int c0 = 0; c0 < p.Cin; c0 += p.Cc) {
    const int cvalid = min(p.Cc, p.Cin - c0);
    PROF(0)
    __syncthreads();
    PROF(1)
    PROF_WAITV()
    PROF(8)
    if (XFK == LXF_COND) {
      // stage this chunk's W0x rows, then compute lrelu(cv0) for the chunk with MFMA: D[t][c] = E[t][k] * W0x[k][c]
      const int kv = p.Cv * 3;
      for (int idx = tid; idx < p.Cc * kv; idx += 256) {
        const int c = idx / kv, k = idx - c * kv;
        wx[c * WX + k] = (c < cvalid) ? p.cw[(long)(c0 + c) * p.cw_stride + k] : 0.f;
      }
      __syncthreads();
      const int ntl = p.Cc >> 4;                          // channel tiles of 16 (Cc is 16 or 32)
      float k3v[2][3];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int c = c0 + nt * 16 + ln;
        const bool cv = nt < ntl && (nt * 16 + ln) < cvalid;
#pragma unroll
        for (int e = 0; e < 3; ++e) k3v[nt][e] = cv ? p.k3[((long)b * p.Cin + c) * 3 + e] : 0.f;
      }
      const int mtl = (p.span + 15) >> 4;
      // per-lane operands of the pre-pass that do not depend on the time tile: the (channel, tap) walk of the A operand
      // and the whole B operand (W0x chunk) live in registers for all the time tiles of this chunk
      int eoff[6]; float bwr[2][6];
#pragma unroll
      for (int st = 0; st < 6; ++st) {
        const int k = st * 4 + kq;
        const int ce = (k * 11) >> 5;                       // k / 3 for k < 32
        eoff[st] = (k < kv) ? ce * p.ES + (k - ce * 3) : -1;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) bwr[nt][st] = (nt < ntl && k < kv) ? wx[(nt * 16 + ln) * WX + k] : 0.f;
      }
      for (int mtile = wave; mtile < mtl; mtile += 4) {
        f32x4 pa[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
        const float* ep = es + mtile * 16 + ln;
#pragma unroll
        for (int st = 0; st < 6; ++st) {
          if (st * 4 < kv) {
            const float a = eoff[st] >= 0 ? ep[eoff[st]] : 0.f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
              if (nt >= ntl) continue;
              pa[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bwr[nt][st], pa[nt], 0, 0, 0);
            }
          }
        }
        const int t0 = mtile * 16 + kq * 4;                 // lane owns 4 consecutive positions of channel (nt*16 + ln)
        if (t0 < p.span) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            if (nt >= ntl) continue;
            const int cl = nt * 16 + ln;
            f32x4 raw, act;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int pos = q0 + t0 + r;
              const bool inside = pos >= 0 && pos < p.T && cl < cvalid;
              const float v = pa[nt][r] + (pos == 0 ? k3v[nt][0] : (pos == p.T - 1 ? k3v[nt][2] : k3v[nt][1]));
              raw[r] = inside ? v : 0.f;
              act[r] = inside ? fmaxf(v, v * p.slope) * p.in_scale : 0.f;
            }
            *reinterpret_cast<f32x4*>(xs + cl * p.XS + t0) = act;
            // the block row 0 of each time tile also materialises cv0 (own columns only) for the backward pass
            const int pos0 = q0 + t0;
            if (p.cv0 && by == 0 && cl < cvalid && pos0 >= n0 && pos0 < n0 + NT && pos0 < p.T)
              *reinterpret_cast<f32x4*>(p.cv0 + (long)b * p.cv0_bs + (long)(c0 + cl) * p.T + pos0) = raw;
          }
        }
      }
    } else if (xpipe) {
      walk_commit_act<XVP>(xr, xw, p.xnp, xs, p.slope, p.in_scale, tail);
      if (end_tile && p.reflect) {   // reflect halo of the first / last tile: columns with q < 0 or q >= T
        const int nl = q0 < 0 ? -q0 : 0;
        const int rfirst = p.T - q0;                       // first column index with q >= T
        const int nr = rfirst < p.span ? p.span - rfirst : 0;
        const int nh = nl + nr;
        __syncthreads();                                   // the zero-filled halo columns were written by other threads
        const float* xc = xrow0 + (long)c0 * p.T;
        const float inv = 1.0f / (float)nh;
        for (int e = tid; e < cvalid * nh; e += 256) {
          const int r = (int)(((float)e + 0.5f) * inv);
          const int h = e - r * nh;
          const int i = h < nl ? h : rfirst + (h - nl);
          int q = q0 + i;
          q = q < 0 ? -q : 2 * (p.T - 1) - q;
          float v = (q >= 0 && q < p.T) ? xc[(long)r * p.T + q] : 0.f;
          v = (v > 0.f ? v : v * p.slope) * p.in_scale;
          xs[r * p.XS + i] = v;
        }
      }
    } else if (interior) {   // FiLM / activation-mask prologues: batches of 4 passes, up to three tensors in flight
      const int xbytes = (p.Cin - c0) * p.T * 4 + fold_bytes;
      const srd_t rx = make_srd(xrow0 + (long)c0 * p.T, xbytes);
      const srd_t ra = make_srd(arow0 + (long)c0 * p.T, xbytes);
      const srd_t rb = make_srd(arow0 + (long)(p.Cin + c0) * p.T, XFK == LXF_FILM ? xbytes : 0);
      int vo = xw.voff;
      float* dst = xs + xw.loff;
      for (int pb = 0; pb < p.xnp; pb += 4) {
        f32x4 t[4], a[4], c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (pb + i < p.xnp) {
            t[i] = buf_load4(rx, vo); a[i] = buf_load4(ra, vo);
            if (XFK == LXF_FILM) c[i] = buf_load4(rb, vo);
            vo += xw.gstep;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (pb + i < p.xnp) {
            f32x4 v = t[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (XFK == LXF_FILM) { const float h = v[q] * (1.f + a[i][q]) + c[i][q]; v[q] = fmaxf(h, h * p.slope); }
              else if (XFK == LXF_MASK_LRELU) v[q] = a[i][q] > 0.f ? v[q] : v[q] * p.slope;
              else v[q] = v[q] * (1.f - a[i][q] * a[i][q]);
              v[q] *= p.in_scale;
              if (tail && q >= xw.nk) v[q] = 0.f;
            }
            if (xw.active) *reinterpret_cast<f32x4*>(dst) = v;
            dst += xw.lstep;
          }
        }
      }
    } else {   // edge tile: per-element padding logic
      for (int r = wave; r < p.Cc; r += 4) {
        float* row = xs + r * p.XS;
        const bool rv = r < cvalid;
        for (int i = lane; i < p.span; i += 64) row[i] = rv ? lean_fetch<(XFK == LXF_COND ? LXF_ACT : XFK)>(p, b, c0 + r, q0 + i) : 0.f;
      }
    }
    walk_commit_w<WVP>(wr, ww, p.wnp, ws);
    PROF(2)
    __syncthreads();
    PROF(3)
    if (c0 + p.Cc < p.Cin) {
      if (xpipe) x_issue(c0 + p.Cc);
      w_issue(c0 + p.Cc);
    }
    PROF(4)

    // MFMA: D[t][co] += X'[t][k] * W[k][co]; one step = 4 channels of one tap. Fragments of step s+1 are
    // read from LDS into the other register set before the MFMAs of step s issue (software pipelining);
    // the (tap, channel-group) walk is kept in scalar registers so a step costs 1 + M_REP vector adds.
    const int csteps = cvalid >> 2;                        // rows past cvalid are never read (Cin % 4 == 0)
    const int nsteps = p.K * csteps;
    const float* w_lane = ws + (wrow0 + ln) * p.WS + kq * p.K;
    const float* x_lane = xs + kq * p.XS + wcol0 + ln + p.i0;
    const int wrep = 16 * p.WS;
    int sj = 0, scs = 0;                                   // scalar walk state
    int woff = p.flip ? p.K - 1 : 0, xoff = 0;
    auto advance = [&]() {
      if (++scs == csteps) { scs = 0; ++sj; woff = p.flip ? p.K - 1 - sj : sj; xoff = sj * p.d; }
      else { woff += 4 * p.K; xoff += 4 * p.XS; }
    };
    constexpr int DEPTH = lean_ring_depth(M_REP, N_REP);
    constexpr int NSET = DEPTH > 2 ? DEPTH : 2;
    float wv[NSET][M_REP], xv[NSET][N_REP];
    int noff[N_REP];                                       // LDS column of sub-tile n relative to the wave's first column
#pragma unroll
    for (int n = 0; n < N_REP; ++n) {
      const int col = wcol0 + n * 16;
      noff[n] = FOLD ? (col / p.T) * p.seg + (col % p.T) - wcol0 : n * 16;
    }
    auto load_frag = [&](int buf) {
      const float* wp = w_lane + woff;
      const float* xp = x_lane + xoff;
#pragma unroll
      for (int m = 0; m < M_REP; ++m) wv[buf][m] = wp[m * wrep];
#pragma unroll
      for (int n = 0; n < N_REP; ++n) xv[buf][n] = xp[FOLD ? noff[n] : n * 16];
    };
    auto mma = [&](int buf) {
#pragma unroll
      for (int m = 0; m < M_REP; ++m)
#pragma unroll
        for (int n = 0; n < N_REP; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[buf][n], wv[buf][m], acc[m][n], 0, 0, 0);
    };
    // Fragment ring (tiles with one or two MFMAs per step), run once per tap over its n channel groups: a slot is one step's
    // fragments. The n % DEPTH odd steps run first: their reads go out together, then their MFMAs. The other steps run in rounds of
    // DEPTH: the reads of the first round go out up front, each later round runs the MFMAs of slot i and refills it with the step
    // DEPTH ahead, the last round only drains. Each stage is straight-line code with fixed slot registers, so the wait in front of
    // an MFMA counts the younger reads still in flight (a wait the compiler places behind a branch merge is lgkmcnt(0)). No read
    // is issued for a step >= n. issue() reads at its cursor and advances it; use() takes the slots in order.
    auto ring_run = [&](const int n, auto&& issue, auto&& use) {
      const int rounds = n / DEPTH, odd = n - rounds * DEPTH;
#pragma unroll
      for (int i = 0; i < DEPTH - 1; ++i)
        if (i < odd) issue(i);
#pragma unroll
      for (int i = 0; i < DEPTH - 1; ++i)
        if (i < odd) use(i);
      if (rounds > 0) {
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) issue(i);
        for (int r = 1; r < rounds; ++r) {
#pragma unroll
          for (int i = 0; i < DEPTH; ++i) {
            use(i); issue(i);
            __builtin_amdgcn_sched_barrier(0);             // keep the steps apart: grouped, the reads of a whole round wait behind one lgkmcnt(0)
          }
        }
#pragma unroll
        for (int i = 0; i < DEPTH; ++i) use(i);
      }
    };
    auto one_ahead_run = [&]() {
      load_frag(0);
      int s = 0;
      for (; s + 2 <= nsteps; s += 2) {
        advance(); load_frag(1);
        mma(0);
        if (s + 2 < nsteps) { advance(); load_frag(0); }
        mma(1);
      }
      if (s < nsteps) mma(0);
    };
    if constexpr (DEPTH == 0) one_ahead_run();
    else if (p.one_ahead) one_ahead_run();                 // test-only (tdvc_debug_knob 8): the ring's results are compared with this loop's
    else {
      for (int j = 0; j < p.K; ++j) {   // one ring per tap: a step's walk is a bump of the two lane addresses, nothing scalar
        const float* wp = w_lane + (p.flip ? p.K - 1 - j : j);
        const float* xp = x_lane + j * p.d;
        ring_run(csteps, [&](int slot) {
#pragma unroll
          for (int m = 0; m < M_REP; ++m) wv[slot][m] = wp[m * wrep];
#pragma unroll
          for (int n = 0; n < N_REP; ++n) xv[slot][n] = xp[FOLD ? noff[n] : n * 16];
          wp += 4 * p.K; xp += 4 * p.XS;
        }, mma);
      }
    }

    // Reflect-pad fold (input-grad of a reflect conv), edge waves only: the gradient of the mirrored halo columns is added to the
    // columns they mirror. At tap j the mirrored column u reads the staged tile at position base - u + j * d, base = -pad on the left
    // side and 2 (T - 1) - pad on the right; a position outside [0, T) holds the zeros the staging wrote. fold_taps gives, for the
    // 16-column sub-tile that starts at column ca, the taps [jlo, jhi] at which some mirrored column [ua, ub] of the sub-tile reads
    // inside the sequence (j * d >= ua - base for the first, j * d <= T - 1 - base + ub for the last; with 'same' padding at most
    // (K - 1) / 2 of the K taps, and 2 of 11 on the second sub-tile of K = 11, d = 5), and false when the sub-tile holds no mirrored
    // column or no such tap. The loops below run over these taps only: the steps they leave out added zero products to sums that
    // started at +0 and so never hold -0, and no bit moves. Wave-uniform, kept in scalar registers (the divisions are exact in fp32: numerators <= K * d).
    // The range is worked out where it is used, per chunk: it depends on nothing the chunk loop changes, and hoisted in front of the
    // main loop the ranges of every (side, sub-tile) cost the tiles that sit at their register limit scratch or a resident block
    // (the empty asm keeps the sub-tile's column, and all that follows from it, inside the loop).
    // p.full_fold (test-only, tdvc_debug_knob 10): every tap, and on the 16-row tiles every sub-tile -- the fold as it was.
    auto fold_taps = [&](const int side, const int n, int& ca, int& jlo, int& jhi) __attribute__((always_inline)) -> bool {
      ca = __builtin_amdgcn_readfirstlane(n0 + wcol0 + n * 16);
      int dd = p.d;
      asm volatile("" : "+s"(ca), "+s"(dd));
      const float inv_d = 1.0f / (float)dd;
      const int cb = ca + 15;
      int ua, ub, base;
      if (side == 0) { ua = max(ca, 1); ub = min(min(cb, p.mirror), p.T - 1); base = -p.pad; }
      else { ua = max(max(ca, p.T - 1 - p.mirror), 0); ub = min(cb, p.T - 2); base = 2 * (p.T - 1) - p.pad; }
      const int nlo = ua - base, nhi = p.T - 1 - base + ub, kd = (p.K - 1) * dd;
      int lo = nlo <= 0 ? 0 : (int)(((float)(min(nlo, kd + dd) + dd - 1) + 0.5f) * inv_d);
      int hi = nhi < 0 ? -1 : (int)(((float)min(nhi, kd) + 0.5f) * inv_d);
      bool use = ua <= ub && lo <= hi;
      if (p.full_fold) {
        use = M_REP == 1 || (side == 0 ? (ca <= p.mirror && cb >= 1) : (ca <= p.T - 2 && cb >= p.T - 1 - p.mirror));
        lo = 0; hi = p.K - 1;
      }
      jlo = __builtin_amdgcn_readfirstlane(lo); jhi = __builtin_amdgcn_readfirstlane(hi);
      return __builtin_amdgcn_readfirstlane((int)use) != 0;
    };
    if (M_REP >= 2 && (needL || needR)) {
      // Per side, only the 16-column sub-tiles that hold mirrored columns take part (pad <= 25: one or two of them). Each
      // runs a software-pipelined (tap, channel-group) loop into a temporary accumulator that is then added to the
      // sub-tile's own accumulators, so the extra work of the blocks at the sequence ends stays a fraction of a chunk.
      for (int side = 0; side < 2; ++side) {
        if (side == 0 ? !needL : !needR) continue;
#pragma unroll
        for (int n = 0; n < N_REP; ++n) {
          int ca, jlo, jhi;
          if (!fold_taps(side, n, ca, jlo, jhi)) continue;
          const int u = ca + ln;
          bool mv; int mb;
          if (side == 0) { mv = (u >= 1 && u <= p.mirror && u < p.T); mb = -u - n0 + p.i0; }
          else { mv = (u >= p.T - 1 - p.mirror && u <= p.T - 2 && u >= 0); mb = 2 * (p.T - 1) - u - n0 + p.i0; }
          f32x4 tacc[M_REP];
#pragma unroll
          for (int m = 0; m < M_REP; ++m) tacc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
          const int nit = (jhi - jlo + 1) * csteps;
          float wq[2][M_REP], xq[2];
          int mj = jlo, mcs = 0;
          auto mload = [&](int buf) {
            const float* wj = w_lane + (p.flip ? p.K - 1 - mj : mj) + mcs * 4 * p.K;
#pragma unroll
            for (int m = 0; m < M_REP; ++m) wq[buf][m] = wj[m * wrep];
            const int idx = mb + mj * p.d;
            const bool ok = mv && idx >= 0 && idx < p.span;
            const float t = xs[(mcs * 4 + kq) * p.XS + (ok ? idx : 0)];
            xq[buf] = ok ? t : 0.f;
            if (++mcs == csteps) { mcs = 0; ++mj; }
          };
          mload(0);
          for (int it = 0; it < nit; it += 2) {
            if (it + 1 < nit) mload(1);
#pragma unroll
            for (int m = 0; m < M_REP; ++m) tacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xq[0], wq[0][m], tacc[m], 0, 0, 0);
            if (it + 1 < nit) {
              if (it + 2 < nit) mload(0);
#pragma unroll
              for (int m = 0; m < M_REP; ++m) tacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xq[1], wq[1][m], tacc[m], 0, 0, 0);
            }
          }
#pragma unroll
          for (int m = 0; m < M_REP; ++m) acc[m][n] += tacc[m];
        }
      }
    }
    if (M_REP == 1 && (needL || needR)) {   // reflect-pad fold, 16-row tiles: sub-tile by sub-tile, straight into its accumulators
      for (int side = 0; side < 2; ++side) {
        if (side == 0 ? !needL : !needR) continue;
#pragma unroll
        for (int n = 0; n < N_REP; ++n) {
          int ca, jlo, jhi;
          if (!fold_taps(side, n, ca, jlo, jhi)) continue;
          const int u = ca + ln;
          bool mv; int mb;
          if (side == 0) { mv = (u >= 1 && u <= p.mirror && u < p.T); mb = -u - n0 + p.i0; }
          else { mv = (u >= p.T - 1 - p.mirror && u <= p.T - 2 && u >= 0); mb = 2 * (p.T - 1) - u - n0 + p.i0; }
          if constexpr (DEPTH > 0) {
            if (!p.one_ahead) {   // a ring per live tap here too: the clamped column and the lanes' `ok` are the tap's
              const int mbv = mv ? mb : -(1 << 28);            // lanes without a mirrored column: an origin no tap brings into [0, span)
              for (int j = jlo; j <= jhi; ++j) {
                const float* wp = w_lane + (p.flip ? p.K - 1 - j : j);
                const int idx = mbv + j * p.d;
                const bool ok = (unsigned)idx < (unsigned)p.span;
                const float* xp = xs + kq * p.XS + (ok ? idx : 0);
                ring_run(csteps, [&](int slot) {
#pragma unroll
                  for (int m = 0; m < M_REP; ++m) wv[slot][m] = wp[m * wrep];
                  xv[slot][n] = *xp; xp += 4 * p.XS;
                  wp += 4 * p.K;
                }, [&](int slot) {
#pragma unroll
                  for (int m = 0; m < M_REP; ++m)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? xv[slot][n] : 0.f, wv[slot][m], acc[m][n], 0, 0, 0);
                });
              }
              continue;
            }
          }
          for (int j = jlo; j <= jhi; ++j) {   // plain loop (from four MFMAs per step on; test-only for the ring's tiles)
            const float* wj = w_lane + (p.flip ? p.K - 1 - j : j);
            const int idx = mb + j * p.d;
            const bool ok = mv && idx >= 0 && idx < p.span;
            for (int cs = 0; cs < csteps; ++cs) {
              float wm_[M_REP];
#pragma unroll
              for (int m = 0; m < M_REP; ++m) wm_[m] = wj[m * 16 * p.WS + cs * 4 * p.K];
              const float t = xs[(cs * 4 + kq) * p.XS + (ok ? idx : 0)];
              const float xm_ = ok ? t : 0.f;
#pragma unroll
              for (int m = 0; m < M_REP; ++m)
                acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xm_, wm_[m], acc[m][n], 0, 0, 0);
            }
          }
        }
      }
    }
    PROF(5)
  }

  // ---- epilogue: lane owns channel co = .. + ln and time steps t0 .. t0+3 (t0 % 4 == 0, T % 4 == 0)
  auto sign_nibble = [](const f32x4& v, const int t0) -> unsigned {   // this float4's sign bits at their place in the 32-step word
    return ((v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u)) << (t0 & 31);
  };
  if (p.old_epi) {   // test-only (tdvc_debug_knob 9): one float4 at a time, every operand load behind its own test -- the batched epilogue's results are compared with this one's
    if (!vec_ok) {   // short, unaligned sequences (T = 50, 63): scalar epilogue
#pragma unroll
      for (int m = 0; m < M_REP; ++m) {
        const int co = r0 + wrow0 + m * 16 + ln;
        if (co >= p.Cout) continue;
        const long ro = (long)co * p.T;
        const float bias = (EPI == EPI_FWD && p.bias) ? p.bias[co] : 0.f;
#pragma unroll
        for (int n = 0; n < N_REP; ++n) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int t = n0 + wcol0 + n * 16 + kq * 4 + q;
            if (t >= p.T) continue;
            const long oi = ro + t;
            float v = acc[m][n][q];
            if (EPI == EPI_FWD) {
              v += bias;
              if (p.bias3) v += p.bias3[((long)b * p.Cout + co) * 3 + (t == 0 ? 0 : (t == p.T - 1 ? 2 : 1))];
              if (p.res) v += p.res[(long)b * p.res_bs + oi];
              if (p.post == POST_LRELU) v = fmaxf(v, v * p.m_slope);
              else if (p.post == POST_TANH) v = tanhf(v);
              v *= p.out_scale;
            } else if (EPI == EPI_MASK) {
              v = p.mx[(long)b * p.mx_bs + oi] > 0.f ? v : v * p.m_slope;
            } else if (EPI == EPI_FILM) {
              const float h = p.mx[(long)b * p.mx_bs + oi];
              const float* gp = p.gb + (long)b * p.gb_bs + oi;
              const float ga = gp[0], be = gp[(long)p.Cout * p.T];
              const float dh2 = (h * (1.f + ga) + be) > 0.f ? v : v * p.m_slope;
              float* dg = p.dgb + (long)b * p.dgb_bs + oi;
              dg[0] = dh2 * h; dg[(long)p.Cout * p.T] = dh2;
              v = dh2 * (1.f + ga);
            }
            if (p.add) v += p.add_scale * p.add[(long)b * p.add_bs + oi];
            p.y[(long)b * p.y_bs + oi] = v;
          }
        }
      }
    } else {
      // One float4 of the output: channel co, time steps t0 .. t0+3 (all inside the tensor). Returns the stored values.
      auto epi_store = [&](f32x4 v, const int co, const int t0, const float bias, const int b) -> f32x4 {     // b: the sample (shadows the block's)
        const long oi = (long)co * p.T + t0;
        if (EPI == EPI_FWD) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] += bias;
          if (p.bias3) {
            const float* k3 = p.bias3 + ((long)b * p.Cout + co) * 3;
            const float mid = k3[1];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += mid;
            if (t0 == 0) v[0] += k3[0] - mid;
            if (t0 + 4 == p.T) v[3] += k3[2] - mid;
          }
          if (p.res) { const f32x4 r = *reinterpret_cast<const f32x4*>(p.res + (long)b * p.res_bs + oi); v += r; }
          if (p.post == POST_LRELU) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], v[q] * p.m_slope);
          } else if (p.post == POST_TANH) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = tanhf(v[q]);
          }
          v *= p.out_scale;
        } else if (EPI == EPI_MASK) {
          if (N_REP >= 2 && p.mbits) {   // sign bits instead of the fp32 mask source: one word per 32 time steps (host: T % 32 == 0)
            const unsigned wbits = p.mbits[(long)b * p.mb_bs + (long)co * (p.T >> 5) + (t0 >> 5)] >> (t0 & 31);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = ((wbits >> q) & 1u) ? v[q] : v[q] * p.m_slope;
          } else {
            const f32x4 mm = *reinterpret_cast<const f32x4*>(p.mx + (long)b * p.mx_bs + oi);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = mm[q] > 0.f ? v[q] : v[q] * p.m_slope;
          }
        } else if (EPI == EPI_FILM) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(p.mx + (long)b * p.mx_bs + oi);
          const float* gp = p.gb + (long)b * p.gb_bs + oi;
          const f32x4 ga = *reinterpret_cast<const f32x4*>(gp);
          const f32x4 be = *reinterpret_cast<const f32x4*>(gp + (long)p.Cout * p.T);
          f32x4 dga, dbe;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float h2 = h[q] * (1.f + ga[q]) + be[q];
            const float dh2 = h2 > 0.f ? v[q] : v[q] * p.m_slope;
            dga[q] = dh2 * h[q]; dbe[q] = dh2; v[q] = dh2 * (1.f + ga[q]);
          }
          float* dg = p.dgb + (long)b * p.dgb_bs + oi;
          *reinterpret_cast<f32x4*>(dg) = dga;
          *reinterpret_cast<f32x4*>(dg + (long)p.Cout * p.T) = dbe;
        }
        if (p.add) { const f32x4 a4 = *reinterpret_cast<const f32x4*>(p.add + (long)b * p.add_bs + oi); v += a4 * p.add_scale; }
        *reinterpret_cast<f32x4*>(p.y + (long)b * p.y_bs + oi) = v;
        return v;
      };
#pragma unroll
      for (int m = 0; m < M_REP; ++m) {
        const int co = r0 + wrow0 + m * 16 + ln;
        if (co >= p.Cout) continue;
        float bias = 0.f;
        if (EPI == EPI_FWD && p.bias) bias = p.bias[co];
        unsigned sb_word = 0;
#pragma unroll
        for (int n = 0; n < N_REP; ++n) {
          int t0 = n0 + wcol0 + n * 16 + kq * 4, bb = b;
          if (FOLD) { const int sg = t0 / p.T; t0 -= sg * p.T; bb = b + sg; if (bb >= p.Bn) continue; }
          if (t0 >= p.T) continue;
          const f32x4 v = epi_store(acc[m][n], co, t0, bias, bb);
          if (EPI == EPI_FWD && N_REP >= 2 && p.sbits) {
            // sign bits of the stored values: the 4 lanes (kq = 0..3) of a channel are OR-ed with two wave shuffles, and sub-tiles
            // (n, n+1) make one 32-bit word (the wave's first column is a multiple of 32: 16 * N_REP columns per wave, N_REP even)
            const unsigned h = sign_nibble(v, t0);
            sb_word = (n & 1) ? (sb_word | h) : h;
            if (n & 1) {
              unsigned w = sb_word;
              w |= (unsigned)__shfl_xor((int)w, 16);
              w |= (unsigned)__shfl_xor((int)w, 32);
              if (kq == 0) p.sbits[(long)b * p.sb_bs + (long)co * (p.T >> 5) + (t0 >> 5)] = w;
            }
          }
        }
      }
    }
    PROF(6)
    PROF_END
    return;
  }
  // Batched epilogue. A batch is EB rows of the wave's sub-tiles (lean_epi_rows: the whole tile on the 16-row tiles). The loads of a
  // whole batch go out first, then each float4 is computed and stored in the old order, with the old expressions. No load and no
  // store stands behind a branch: a lane past Cout, past T or past the last sample of a folded group carries an out-of-range buffer
  // offset instead, which loads zeros and drops the store. What changes the code is resolved once per block, in front of the batches,
  // and each answer enters its own straight-line code: float4 or dword accesses, with or without add, fp32 or 1-bit mask, the
  // post-activation. (add is part of the code because `v * scale + add * add_scale` contracts to another FMA when v has a second
  // use.) The forward's res and bias3 only ever follow additions: an absent one has an empty descriptor, so its loads fetch nothing,
  // and its term is kept out of the sum by a select on the wave-uniform flag (no added zero: -0.0 + 0.0 would move a bit).
  // (Tested per float4, on pointers that may alias the stores, every operand load was followed by s_waitcnt vmcnt(0) -- which on
  // this ISA also waits for the store in front: up to 32 exposed memory round trips per wave behind the last MFMA.) The scalar path
  // (rows not 16-byte aligned: T = 50, 63) runs the same batches with four dword accesses per operand.
  constexpr int EB = lean_epi_rows(M_REP, N_REP, EPI), NB = lean_epi_cols(M_REP, N_REP, WM, XFK, EPI);
  constexpr int OOR = 0x7f000000;
  const int ct = p.Cout * p.T;
  const int nsamp = FOLD ? min(p.fold, p.Bn - b) : 1;      // samples of the tile that exist
  const bool has_res = EPI == EPI_FWD && p.res != nullptr, has_b3 = EPI == EPI_FWD && p.bias3 != nullptr;
  auto srd_of = [&](const float* base, int bs, bool has) __attribute__((always_inline)) {   // one [B][Cout][T] operand over the tile's samples
    return make_srd(has ? base + (long)b * bs : nullptr, has ? ((nsamp - 1) * bs + ct) * 4 : 0);
  };
  auto epilogue = [&](auto VEC_, auto ADD_, auto BITS_, auto POST_) __attribute__((always_inline)) {
    constexpr bool VEC = decltype(VEC_)::value, ADD = decltype(ADD_)::value, BITS = decltype(BITS_)::value;
    constexpr int POST = decltype(POST_)::value;
    constexpr bool MX = (EPI == EPI_MASK && !BITS) || EPI == EPI_FILM;
    const srd_t sy = srd_of(p.y, p.y_bs, true), sadd = srd_of(p.add, p.add_bs, ADD), sres = srd_of(p.res, p.res_bs, has_res);
    const srd_t smx = srd_of(p.mx, p.mx_bs, MX);
    const srd_t sga = srd_of(p.gb, p.gb_bs, EPI == EPI_FILM), sbe = srd_of(p.gb + ct, p.gb_bs, EPI == EPI_FILM);
    const srd_t sdg = srd_of(p.dgb, p.dgb_bs, EPI == EPI_FILM), sdb = srd_of(p.dgb + ct, p.dgb_bs, EPI == EPI_FILM);
    const srd_t sbit = make_srd(BITS ? reinterpret_cast<const float*>(p.mbits + (long)b * p.mb_bs) : nullptr, BITS ? p.Cout * (p.T >> 5) * 4 : 0);
    const srd_t sbias = make_srd(p.bias, (EPI == EPI_FWD && p.bias) ? p.Cout * 4 : 0);
    const srd_t sb3 = make_srd(has_b3 ? p.bias3 + (long)b * p.Cout * 3 : nullptr, has_b3 ? nsamp * p.Cout * 12 : 0);
    // a float4 (VEC) or its four dwords, each inside the row or out of range
    auto ld = [&](const srd_t s, const int o, const int t0) __attribute__((always_inline)) -> f32x4 {
      if constexpr (VEC) return buf_load4(s, o);
      else {
        f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = buf_load1(s, (o != OOR && t0 + q < p.T) ? o + 4 * q : OOR);
        return r;
      }
    };
    auto st = [&](const srd_t s, const int o, const int t0, const f32x4 v) __attribute__((always_inline)) {
      if constexpr (VEC) buf_store4(s, o, v);
      else {
#pragma unroll
        for (int q = 0; q < 4; ++q) buf_store1(s, (o != OOR && t0 + q < p.T) ? o + 4 * q : OOR, v[q]);
      }
    };
#pragma unroll
    for (int m0 = 0; m0 < M_REP; m0 += EB) {
      int tt[N_REP], sg[N_REP], off[EB][N_REP];
      bool ok[EB][N_REP];
      f32x4 vmx[EB][N_REP], vadd[EB][N_REP], vres[EB][N_REP], vga[EB][N_REP], vbe[EB][N_REP];
      unsigned wb[EB][N_REP];
      float bias[EB], k3v[EB][FOLD ? N_REP : 1][3];      // bias and bias3: once per row and sample
      // byte offset of the float4 in an operand with batch stride bs
      auto at = [&](int mi, int n, int bs) __attribute__((always_inline)) { return FOLD ? (ok[mi][n] ? off[mi][n] + sg[n] * bs * 4 : OOR) : off[mi][n]; };
#pragma unroll
      for (int n = 0; n < N_REP; ++n) {
        tt[n] = n0 + wcol0 + n * 16 + kq * 4; sg[n] = 0;
        if (FOLD) { sg[n] = tt[n] / p.T; tt[n] -= sg[n] * p.T; }
      }
#pragma unroll
      for (int nb = 0; nb < N_REP; nb += NB) {
        // ---- issue: every load of the batch
#pragma unroll
        for (int mi = 0; mi < EB; ++mi) {
          const int co = r0 + wrow0 + (m0 + mi) * 16 + ln;
          if (EPI == EPI_FWD && nb == 0) {
            bias[mi] = buf_load1(sbias, co * 4);
#pragma unroll
            for (int s = 0; s < (FOLD ? N_REP : 1); ++s)
#pragma unroll
              for (int e = 0; e < 3; ++e)
                k3v[mi][s][e] = buf_load1(sb3, (co < p.Cout && sg[s] < nsamp) ? ((sg[s] * p.Cout + co) * 3 + e) * 4 : OOR);
          }
#pragma unroll
          for (int n = nb; n < nb + NB; ++n) {
            ok[mi][n] = co < p.Cout && tt[n] < p.T && (!FOLD || sg[n] < nsamp);
            off[mi][n] = ok[mi][n] ? (co * p.T + tt[n]) * 4 : OOR;
            if (EPI == EPI_FWD) vres[mi][n] = ld(sres, at(mi, n, p.res_bs), tt[n]);
            if constexpr (BITS) wb[mi][n] = __builtin_bit_cast(unsigned, buf_load1(sbit, ok[mi][n] ? (co * (p.T >> 5) + (tt[n] >> 5)) * 4 : OOR));
            if constexpr (MX) vmx[mi][n] = ld(smx, at(mi, n, p.mx_bs), tt[n]);
            if (EPI == EPI_FILM) { vga[mi][n] = ld(sga, at(mi, n, p.gb_bs), tt[n]); vbe[mi][n] = ld(sbe, at(mi, n, p.gb_bs), tt[n]); }
            if constexpr (ADD) vadd[mi][n] = ld(sadd, at(mi, n, p.add_bs), tt[n]);
          }
        }
        // ---- consume: the old arithmetic, float4 by float4
#pragma unroll
        for (int mi = 0; mi < EB; ++mi) {
          const int co = r0 + wrow0 + (m0 + mi) * 16 + ln;
          unsigned sb_word = 0;
#pragma unroll
          for (int n = nb; n < nb + NB; ++n) {
            const int t0 = tt[n];
            f32x4 v = acc[m0 + mi][n];
            if (EPI == EPI_FWD) {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] += bias[mi];
              const float* k3 = k3v[mi][FOLD ? n : 0];
              if constexpr (VEC) {
                const float mid = k3[1];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = has_b3 ? v[q] + mid : v[q];
                v[0] = (has_b3 && t0 == 0) ? v[0] + (k3[0] - mid) : v[0];
                v[3] = (has_b3 && t0 + 4 == p.T) ? v[3] + (k3[2] - mid) : v[3];
              } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = has_b3 ? v[q] + (t0 + q == 0 ? k3[0] : (t0 + q == p.T - 1 ? k3[2] : k3[1])) : v[q];
              }
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] = has_res ? v[q] + vres[mi][n][q] : v[q];
              if constexpr (POST == POST_LRELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], v[q] * p.m_slope);
              } else if constexpr (POST == POST_TANH) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tanhf(v[q]);
              }
              v *= p.out_scale;
            } else if (EPI == EPI_MASK) {
              if constexpr (BITS) {   // sign bits instead of the fp32 mask source: one word per 32 time steps (host: T % 32 == 0)
                const unsigned wbits = wb[mi][n] >> (t0 & 31);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = ((wbits >> q) & 1u) ? v[q] : v[q] * p.m_slope;
              } else {
                const f32x4 mm = vmx[mi][n];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = mm[q] > 0.f ? v[q] : v[q] * p.m_slope;
              }
            } else if (EPI == EPI_FILM) {
              const f32x4 h = vmx[mi][n], ga = vga[mi][n], be = vbe[mi][n];
              f32x4 dga, dbe;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const float h2 = h[q] * (1.f + ga[q]) + be[q];
                const float dh2 = h2 > 0.f ? v[q] : v[q] * p.m_slope;
                dga[q] = dh2 * h[q]; dbe[q] = dh2; v[q] = dh2 * (1.f + ga[q]);
              }
              st(sdg, at(mi, n, p.dgb_bs), t0, dga);
              st(sdb, at(mi, n, p.dgb_bs), t0, dbe);
            }
            if constexpr (ADD) v += vadd[mi][n] * p.add_scale;
            st(sy, at(mi, n, p.y_bs), t0, v);
            if (EPI == EPI_FWD && N_REP >= 2 && p.sbits) {
              // sign bits of the stored values: the 4 lanes (kq = 0..3) of a channel are OR-ed with two wave shuffles, and sub-tiles
              // (n, n+1) make one 32-bit word (the wave's first column is a multiple of 32: 16 * N_REP columns per wave, N_REP even)
              const unsigned h = sign_nibble(v, t0);
              sb_word = (n & 1) ? (sb_word | h) : h;
              if (n & 1) {
                unsigned w = sb_word;
                w |= (unsigned)__shfl_xor((int)w, 16);
                w |= (unsigned)__shfl_xor((int)w, 32);
                if (kq == 0 && ok[mi][n]) p.sbits[(long)b * p.sb_bs + (long)co * (p.T >> 5) + (t0 >> 5)] = w;
              }
            }
          }
        }
      }
    }
  };
  // what changes the code: wave-uniform, resolved here once
  constexpr std::false_type NO{};
  constexpr std::true_type YES{};
  constexpr std::integral_constant<int, POST_NONE> P0{};
  auto by_kind = [&](auto V, auto A) __attribute__((always_inline)) {
    if constexpr (EPI == EPI_FWD) {
      if (p.post == POST_LRELU) epilogue(V, A, NO, std::integral_constant<int, POST_LRELU>{});
      else if (p.post == POST_TANH) epilogue(V, A, NO, std::integral_constant<int, POST_TANH>{});
      else epilogue(V, A, NO, P0);
    } else if constexpr (EPI == EPI_MASK && N_REP >= 2 && decltype(V)::value) {
      if (p.mbits) epilogue(V, A, YES, P0); else epilogue(V, A, NO, P0);
    } else {
      epilogue(V, A, NO, P0);
    }
  };
  if (FOLD || vec_ok) {      // folded tiles are float4 only (host)
    if (p.add) by_kind(YES, YES); else by_kind(YES, NO);
  } else if constexpr (!FOLD) {
    if (p.add) by_kind(NO, YES); else by_kind(NO, NO);
  }
  PROF(6)
  PROF_END
}

// ------------------------------------------------------------------------------------------ host
// Row-walk geometry of a tile of `rows` rows x `nvec` float4: rows per pass and number of passes (conv_common.h RowWalk).
static inline void walk_geometry(int rows, int nvec, int* rp, int* np) {
  *rp = nvec <= 256 ? 256 / nvec : 0;
  if (*rp > rows) *rp = rows;
  *np = *rp ? (rows + *rp - 1) / *rp : 1 << 20;
}

template <int M_REP, int N_REP, int WM, int WN, int XFK, int EPI, bool FOLD = false>
static hipError_t lean_launch3(const LeanP& p, int B, hipStream_t st) {
  constexpr int MT = 16 * M_REP * WM, NT = 16 * N_REP * WN;
  auto k = conv_lean_kernel<M_REP, N_REP, WM, WN, XFK, EPI, FOLD>;
  TDVC_BIG_LDS_ONCE(k); TDVC_TRACE(k);
  dim3 grid(FOLD ? 1 : (p.T + NT - 1) / NT, (p.Cout + MT - 1) / MT, FOLD ? (B + p.fold - 1) / p.fold : B);
  LeanP q = p; q.swz = g_knob[0] && (long)grid.x * grid.y * grid.z >= 16;
  q.one_ahead = g_knob[8] != 0;
  q.old_epi = g_knob[9] != 0;
  q.full_fold = g_knob[10] != 0;
  const size_t lds = (size_t)(p.xnp * p.xrp * p.XS + p.wnp * p.wrp * p.WS) * sizeof(float);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, st, q);
  return hipGetLastError();
}

// folded short-sequence launches (64-column tiles only): the pairs discriminator layer 5 uses
template <int M_REP, int N_REP, int WM, int WN>
static hipError_t lean_launch_fold(const LeanP& p, int B, int xfk, int epi, hipStream_t st) {
  if (xfk == LXF_ACT && epi == EPI_FWD) return lean_launch3<M_REP, N_REP, WM, WN, LXF_ACT, EPI_FWD, true>(p, B, st);
  if (xfk == LXF_ACT && epi == EPI_PLAIN) return lean_launch3<M_REP, N_REP, WM, WN, LXF_ACT, EPI_PLAIN, true>(p, B, st);
  if (xfk == LXF_MASK_LRELU && epi == EPI_PLAIN) return lean_launch3<M_REP, N_REP, WM, WN, LXF_MASK_LRELU, EPI_PLAIN, true>(p, B, st);
  return hipErrorNotSupported;
}

template <int M_REP, int N_REP, int WM, int WN>
static hipError_t lean_launch2(const LeanP& p, int B, int xfk, int epi, hipStream_t st) {
  // the (prologue, epilogue) pairs the train step actually uses; anything else goes to the generic kernel
  if (xfk == LXF_ACT && epi == EPI_FWD) return lean_launch3<M_REP, N_REP, WM, WN, LXF_ACT, EPI_FWD>(p, B, st);
  if (xfk == LXF_FILM && epi == EPI_FWD) return lean_launch3<M_REP, N_REP, WM, WN, LXF_FILM, EPI_FWD>(p, B, st);
  if (xfk == LXF_ACT && epi == EPI_MASK) return lean_launch3<M_REP, N_REP, WM, WN, LXF_ACT, EPI_MASK>(p, B, st);
  if (xfk == LXF_ACT && epi == EPI_FILM) return lean_launch3<M_REP, N_REP, WM, WN, LXF_ACT, EPI_FILM>(p, B, st);
  if (xfk == LXF_ACT && epi == EPI_PLAIN) return lean_launch3<M_REP, N_REP, WM, WN, LXF_ACT, EPI_PLAIN>(p, B, st);
  if (xfk == LXF_MASK_LRELU && epi == EPI_PLAIN) return lean_launch3<M_REP, N_REP, WM, WN, LXF_MASK_LRELU, EPI_PLAIN>(p, B, st);
  return hipErrorNotSupported;
}

// FiLM conditioning forward: gb = cond_var.2(lrelu(cond_var.0(c))) with the cond_var.0 output computed per tile in
// LDS (LXF_COND). p.x = excitation [B][Cv][T]; p.Cin = channels of cv0 (= Cin of cond_var.2); p.w = cond_var.2 weight.
hipError_t launch_conv_lean_cond(LeanP p, int B, hipStream_t st) {
  if ((p.T & 3) || !p.vec || p.K != 3 || p.d != 1 || p.pad != 1 || p.Cv * 3 > 24) return hipErrorNotSupported;
  const int MT = p.Cout <= 32 ? 32 : 64, NT = 256;
  p.mirror = 0; p.flip = 0; p.reflect = 0;
  const int first = -p.pad;
  const int lo = -4;                                   // aligned origin
  p.lo = lo; p.i0 = first - lo;
  p.span = ((NT + (p.K - 1) * p.d - p.pad - lo) + 3) / 4 * 4;
  p.XS = ((p.span + 15) / 32) * 32 + 16;           // smallest stride >= span that is 16 (mod 32): the 4 rows of a fragment read hit disjoint banks
  p.ES = ((p.span + 15) / 16) * 16 + 4;
  int Cc = 32;
  auto geom = [&](int cc) {
    p.Cc = cc; p.WS = p.K * cc + 2;
    p.xrp = cc; p.xnp = 1;                               // the input tile is computed, not loaded: Cc rows
    walk_geometry(MT, p.K * cc / 4, &p.wrp, &p.wnp);
    return (size_t)(cc * p.XS + p.wnp * p.wrp * p.WS + p.Cv * p.ES + cc * 25) * sizeof(float);
  };
  size_t lds = geom(Cc);
  if (lds > (size_t)(g_lds_cap > 0 ? g_lds_cap : 80 * 1024) || p.wnp > (MT >= 48 ? 10 : 6)) lds = geom(Cc = 16);
  dim3 grid((p.T + NT - 1) / NT, (p.Cout + MT - 1) / MT, B);
  p.swz = g_knob[0] && (long)grid.x * grid.y * grid.z >= 16;
  p.old_epi = g_knob[9] != 0;
  if (MT == 32) {
    auto k = conv_lean_kernel<2, 4, 1, 4, LXF_COND, EPI_FWD>;
    TDVC_BIG_LDS_ONCE(k); TDVC_TRACE(k);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, p);
  } else {
    auto k = conv_lean_kernel<4, 4, 1, 4, LXF_COND, EPI_FWD>;
    TDVC_BIG_LDS_ONCE(k); TDVC_TRACE(k);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, p);
  }
  return hipGetLastError();
}

// Returns hipErrorNotSupported when the shape/variant is outside the lean kernel's contract.
hipError_t launch_conv_lean(LeanP p, int B, int xfk, int epi, hipStream_t st) {
  const bool combo = (xfk == LXF_ACT) || (xfk == LXF_FILM && epi == EPI_FWD) || (xfk == LXF_MASK_LRELU && epi == EPI_PLAIN);
  if (!combo) return hipErrorNotSupported;
  // Tile choice: the largest tile whose grid still covers the chip ~2x (256 CUs), else the smallest one.
  struct Cand { int MT, NT, cfg; };
  static const Cand cands[] = {{64, 256, 2}, {48, 256, 5}, {32, 256, 1}, {64, 64, 4}, {32, 64, 6}, {16, 256, 0}, {16, 64, 3}};
  static const Cand tall = {144, 64, 7};     // all 136 rows of cond_var.2's input-grad / cond_var.0 in one block: the input tile is read once
  const int R = p.Cout;
  int MT = 16, NT = 64, cfg = 3;
  for (const Cand& c : cands) {
    if (c.MT > 16 && R <= 16) continue;
    if (c.MT > 32 && R <= 32) continue;
    if (c.MT == 48 && !(R % 64 != 0 && (R + 47) / 48 * 48 < (R + 63) / 64 * 64)) continue;
    if (c.MT == 64 && c.NT == 256 && (R % 64 != 0 && (R + 47) / 48 * 48 < (R + 63) / 64 * 64)) continue;
    if (c.NT == 256 && p.T <= 80) continue;
    const long blocks = (long)((R + c.MT - 1) / c.MT) * ((p.T + c.NT - 1) / c.NT) * B;
    MT = c.MT; NT = c.NT; cfg = c.cfg;
    // 64 x 64 blocks sit 4 to a CU: below one full round of them (D layer 5: exactly 1024) the 32 x 64 tile, with twice
    // the blocks, fills the chip better (128 -> 128 k7 T = 500: 47.7 vs 51.0 us; 136 -> 256 input-grad: 55 vs 61)
    if (blocks >= (c.cfg == 4 ? 1024 : 512)) break;
  }
  // a tiny reduction (the 8-channel excitation window of cond_var.0: Cin*K = 24) makes the conv a pure HBM stream of its
  // output: the 16-row tile keeps the most blocks resident (94 vs 111 us for 8 -> 136, T = 16000, 32 samples)
  if ((long)p.Cin * p.K <= 48 && p.T > 80 && p.mirror == 0) { MT = 16; NT = 256; cfg = 0; }
  // short reductions with many (R = 136: the input-grad of cond_var.2 at the 16/32-channel stages) or few (R = 32)
  // output rows are bound by their epilogue traffic, not by the matrix pipe: 16-row tiles (5 blocks per CU) measured
  // 4-10 % faster than the 48/32-row ones there (profiles/r02_b_tile_sweep.txt)
  if ((long)p.Cin * p.K <= 224 && p.T > 80 && (R >= 128 || R == 32)) { MT = 16; NT = 256; cfg = 0; }
  if (g_force_tile >= 0) {   // test-only (tdvc_debug_force_tile): pin the tile so that small shapes reach every instance
    for (const Cand& c : cands)
      if (c.cfg == g_force_tile) { MT = c.MT; NT = c.NT; cfg = c.cfg; }
    if (g_force_tile == tall.cfg) { MT = tall.MT; NT = tall.NT; cfg = tall.cfg; }
  }
  if (p.sbits || p.mbits) {   // sign-bit words span two 16-column sub-tiles of one wave: not on the tiles with one sub-tile per wave
    if (!p.vec || (p.T & 31) || p.T <= 80) return hipErrorNotSupported;
    if (cfg == 3 || cfg == tall.cfg) { MT = 16; NT = 256; cfg = 0; }
  }
  const int first = -p.pad;
  int lo = -p.pad - p.mirror;
  lo = -(((-lo) + 3) / 4 * 4);
  const int hi = (p.K - 1) * p.d - p.pad + p.mirror;
  p.lo = lo; p.i0 = first - lo;
  p.span = ((NT + hi - lo) + 3) / 4 * 4;
  // short sequences: several samples per 64-column tile (kernel comment at FOLD)
  p.fold = 1; p.seg = 0; p.Bn = B;
  const bool fold_combo = (xfk == LXF_ACT && (epi == EPI_FWD || epi == EPI_PLAIN)) || (xfk == LXF_MASK_LRELU && epi == EPI_PLAIN);
  if (g_knob[4] == 0 && g_force_tile < 0 && NT == 64 && R >= 32 && (p.T == 16 || p.T == 32) && p.Cin % 16 == 0 && B >= 64 / p.T && p.vec && !p.reflect && p.mirror == 0 && fold_combo &&
      !p.sbits && !p.mbits && (!p.aux || p.aux_bs == p.x_bs) && (long)(64 / p.T) * p.x_bs < (1L << 28) &&
      (long)(64 / p.T) * std::max(p.y_bs, std::max(p.res ? p.res_bs : 0, p.add ? p.add_bs : 0)) < (1L << 28)) {   // the epilogue's 32-bit offsets span the group too
    p.fold = 64 / p.T;
    p.seg = ((p.T + hi - lo) + 3) / 4 * 4;
    p.span = p.fold * p.seg;
    // a quarter / half as many blocks as unfolded: take the 32-row tile unless the 64-row one still fills a round of 1024
    const long nb64 = (long)((R + 63) / 64) * ((B + p.fold - 1) / p.fold);
    if (nb64 >= 1024) { MT = 64; cfg = 4; } else { MT = 32; cfg = 6; }
  }
  p.XS = ((p.span + 15) / 32) * 32 + 16;           // smallest stride >= span that is 16 (mod 32): the 4 rows of a fragment read hit disjoint banks
  const int xvp = (MT >= 144 || NT <= 64) ? 4 : (MT >= 32 ? 12 : 6), wvp = MT >= 48 ? 10 : (MT >= 32 ? 6 : 4);   // = the kernel's XVP / WVP
  // LDS budget per block = what lets the blocks the register budget allows (launch_bounds of the instance) actually be
  // resident on a CU with 160 KB: 3 blocks -> 52 KB. With 64 KB only two 32-row x 256-column blocks fit and that kernel
  // ran 22 % slower; the other tiles gain 0-6 % (tools/tile_sweep.py, profiles/r02_b_tile_sweep.txt).
  const size_t lds_cap = g_lds_cap > 0 ? (size_t)g_lds_cap : (size_t)((cfg == 4 ? 40 : 52) * 1024);   // 4 resident 64 x 64 blocks
  int Cc = 0;
  // 16-row tiles over a long reduction (the discriminators' 1024 -> 16 heads: 32 serial chunks of 32 channels on 32-64 blocks, each
  // chunk one exposed load latency: 77 us for 0.2 GFLOP) take chunks of up to 64 channels when the prefetch registers hold them
  const int cc_cap = (MT == 16 && p.Cin >= 256) ? 64 : 32;
  for (int cc = 4; cc <= cc_cap && cc <= ((p.Cin + 3) / 4) * 4; cc += 4) {
    int xrp, xnp, wrp, wnp;
    walk_geometry(cc, p.span / 4, &xrp, &xnp);
    walk_geometry(MT, p.K * cc / 4, &wrp, &wnp);
    const size_t lds = (size_t)(xnp * xrp * p.XS + wnp * wrp * (p.K * cc + 2)) * 4;
    if (lds > lds_cap || wnp > wvp || (xfk == LXF_ACT && xnp > xvp)) continue;
    if (p.fold > 1 && p.Cin % cc) continue;          // folded tiles: whole channel chunks only (a partial one would run into the next sample)
    Cc = cc; p.xrp = xrp; p.xnp = xnp; p.wrp = wrp; p.wnp = wnp;
  }
  if (!Cc) return hipErrorNotSupported;                  // weight tile would not fit the register prefetch
  p.Cc = Cc;
  p.WS = p.K * Cc + 2;
  if (p.fold > 1) return cfg == 4 ? lean_launch_fold<1, 4, 4, 1>(p, B, xfk, epi, st) : lean_launch_fold<1, 2, 2, 2>(p, B, xfk, epi, st);
  switch (cfg) {
    case 0: return lean_launch2<1, 4, 1, 4>(p, B, xfk, epi, st);
    case 1: return lean_launch2<2, 4, 1, 4>(p, B, xfk, epi, st);
    case 2: return lean_launch2<4, 4, 1, 4>(p, B, xfk, epi, st);
    case 3: return lean_launch2<1, 1, 1, 4>(p, B, xfk, epi, st);
    case 5: return lean_launch2<3, 4, 1, 4>(p, B, xfk, epi, st);
    case 6: return lean_launch2<1, 2, 2, 2>(p, B, xfk, epi, st);
    case 7: return lean_launch2<9, 1, 1, 4>(p, B, xfk, epi, st);
    default: return lean_launch2<1, 4, 4, 1>(p, B, xfk, epi, st);
  }
}

}  // namespace tdvc
