// Grouped strided Conv1d with 4 input and 4 output channels per group (model/discriminator.py:26-32, layer 4:
// 1024 -> 1024, kernel 41, stride 4, 256 groups), forward / input-grad / weight-grad on the vector ALU.
//
// Why not the matrix pipe: per group the product is a 4 x 164 by 164 x T matrix product. A 16-row MFMA tile is a quarter
// full, every (group, sample) is its own block of 44 MFMAs, and the 8192-16384 blocks of a launch spend their time in
// staging, barriers and epilogue (profiles/r02_f_generic_conv_phase_cycles.txt: 5 of 23 k cycles in MFMAs; 91 / 127 / 100
// us per launch for fwd / input-grad / weight-grad of a 41 MB problem). Here a wave owns one (group, 64 output steps) and
// a lane one output step: 656 FMAs per lane fed by LDS reads -- the input tile in time-to-depth layout (conflict free),
// the weights as broadcast float4.
// The layers in front of it (4 input, 16 output channels per group) fill the MFMA tile: their forward and input-grad kernels
// (group16_*) are in the second half of this file.
#include "launch.h"
#include "conv_small_group.h"

namespace tdvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// dword load through a raw buffer descriptor: elements that must read as zero get an out-of-range offset, so nothing selects
// on the loaded value and the loads of a batch stay in flight together (conv_common.h: tile_issue)
__device__ __forceinline__ float bload(srd_t rs, int elem, bool ok) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ok ? elem * 4 : 0x7f000000, 0, 0));
}

// ---------------------------------------------------------------------------------------------- forward
// grid (ceil(G / 4), B, ceil(Tout / 64)); wave = one group, lane = one output step.
template <int S>
__global__ __launch_bounds__(256) void small_group_fwd_kernel(const SmallGroupP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x * 4 + wave, b = blockIdx.y, t0 = blockIdx.z * 64;
  const int xsz = 4 * S * p.CS, wsz = 16 * p.K;
  float* xs = smem + wave * (xsz + wsz);          // [ci][phi][CS]
  float* ws = xs + xsz;                           // [ci][k][co]
  const bool live = g < p.G;
  if (live) {
    // All global loads of the wave are issued before the first LDS store (a load -> store loop costs one memory round
    // trip per iteration: 31 of them here).
    // weights: module layout [co][ci][k] -> [ci][k][co]
    const float* wg = p.w + (long)g * 16 * p.K;
    float wv[12];                                  // 16 K <= 768
    const srd_t wrs = make_srd(wg, 16 * p.K * 4);
#pragma unroll
    for (int i = 0; i < 12; ++i) { const int e = lane + i * 64; wv[i] = bload(wrs, e, e < 16 * p.K); }
    // input window: positions q0 .. q0 + span - 1 of the 4 channels, q = q0 + col * s + phi
    const int q0 = t0 * S - p.pad, span = 63 * S + p.K;
    const float inv_s = 1.0f / (float)S;
    const srd_t xrs = make_srd(p.x + (long)b * p.x_bs + (long)(g * 4) * p.Tin, 4 * p.Tin * 4);
    for (int e0 = 0; e0 < span; e0 += 5 * 64) {   // one pass for s = 4, K = 41 (span 293)
      float xv[4][5];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const int e = e0 + lane + i * 64, q = q0 + e;
          xv[ci][i] = bload(xrs, ci * p.Tin + q, e < span && q >= 0 && q < p.Tin);
        }
#pragma unroll
      for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const int e = e0 + lane + i * 64;
          if (e < span) {
            float v = xv[ci][i];
            if (p.act_in) v = fmaxf(v, v * p.slope_in);
            const int col = (int)(((float)e + 0.5f) * inv_s);
            xs[(ci * S + (e - col * S)) * p.CS + col] = v * p.in_scale;
          }
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int e = lane + i * 64;
      if (e < 16 * p.K) { const int co = e / (4 * p.K), r = e - co * 4 * p.K; ws[r * 4 + co] = wv[i]; }   // r = ci * K + k
    }
  }
  __syncthreads();
  if (!live) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ci = 0; ci < 4; ++ci) {
    const float* xc = xs + ci * S * p.CS + lane;
    const f32x4* wc = reinterpret_cast<const f32x4*>(ws) + ci * p.K;
    for (int j = 0; j < p.J; ++j) {               // S taps per step (compile-time stride: no index arithmetic, independent reads)
      float xv4[S]; f32x4 w4[S];
#pragma unroll
      for (int phi = 0; phi < S; ++phi) {
        const bool ok = j * S + phi < p.K;
        // taps past K read columns of the tile that nothing staged (e >= span): mask the OPERAND too -- a zero weight alone
        // would turn a stale Inf / NaN bit pattern in LDS into NaN (0 * x)
        xv4[phi] = ok ? xc[phi * p.CS + j] : 0.f;
        w4[phi] = ok ? wc[j * S + phi] : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int phi = 0; phi < S; ++phi) acc += w4[phi] * xv4[phi];
    }
  }
  const int t = t0 + lane;
  if (t >= p.Tout) return;
#pragma unroll
  for (int co = 0; co < 4; ++co) {
    const int ch = g * 4 + co;
    float v = acc[co] + (p.bias ? p.bias[ch] : 0.f);
    if (p.post == POST_LRELU) v = lrelu_f(v, p.post_slope);
    else if (p.post == POST_TANH) v = tanhf(v);
    p.y[(long)b * p.y_bs + (long)ch * p.Tout + t] = v * p.out_scale;
  }
}

// ---------------------------------------------------------------------------------------------- input-grad
// dx[ci][m*s + r - pad] = sum_{co, j} w[co][ci][r + j*s] * dyM[co][m - j]: a lane owns one m and all s phases r, i.e. s
// consecutive input positions (one float4 store per channel when s == 4).
// grid (ceil(G / 4), B, ceil(M / 64)), M = number of m values = (Tin - 1 + pad) / s + 1.
template <int S>
__global__ __launch_bounds__(256) void small_group_dgrad_kernel(const SmallGroupP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x * 4 + wave, b = blockIdx.y, m0 = blockIdx.z * 64;
  const int DS = 64 + p.J;                         // dyM window [m0 - J + 1, m0 + 63] per output channel
  const int dsz = 4 * DS, wsz = 16 * p.J * S;
  float* ds = smem + wave * (dsz + wsz);          // [co][DS]
  float* ws = ds + dsz;                           // [co][j][r][ci]   (zero for r + j*s >= K)
  const bool live = g < p.G;
  if (live) {
    const float* wg = p.w + (long)g * 16 * p.K;
    float wv[12];                                  // 16 J s <= 768 (host-checked)
    const srd_t wrs = make_srd(wg, 16 * p.K * 4);
    const srd_t drs = make_srd(p.dy + (long)b * p.dy_bs + (long)(g * 4) * p.Tout, 4 * p.Tout * 4);
    const srd_t mrs = make_srd(p.mask ? p.mask + (long)b * p.mask_bs + (long)(g * 4) * p.Tout : p.dy, p.mask ? 4 * p.Tout * 4 : 0);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int e = lane + i * 64;
      const int ci = e & 3; int rest = e >> 2;
      const int r = rest % S; rest /= S;
      const int j = rest % p.J, co = rest / p.J;
      const int k = r + j * S;
      wv[i] = bload(wrs, (co * 4 + ci) * p.K + k, e < wsz && k < p.K);
    }
    float dv[4][2], mv[4][2];                      // DS <= 128
#pragma unroll
    for (int co = 0; co < 4; ++co)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = lane + i * 64, t = m0 - p.J + 1 + e;
        const bool ok = e < DS && t >= 0 && t < p.Tout;
        dv[co][i] = bload(drs, co * p.Tout + t, ok);
        mv[co][i] = bload(mrs, co * p.Tout + t, ok);      // no mask: the empty descriptor reads 0 -> handled below
      }
#pragma unroll
    for (int i = 0; i < 12; ++i) { const int e = lane + i * 64; if (e < wsz) ws[e] = wv[i]; }
#pragma unroll
    for (int co = 0; co < 4; ++co)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = lane + i * 64;
        if (e < DS) { const float v = dv[co][i] * p.dy_scale; ds[co * DS + e] = (!p.mask || mv[co][i] > 0.f) ? v : v * p.m_slope; }
      }
  }
  __syncthreads();
  if (!live) return;
  f32x4 acc[S];                                   // [r] -> 4 input channels
#pragma unroll
  for (int r = 0; r < S; ++r) acc[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int co = 0; co < 4; ++co) {
    const float* dc = ds + co * DS + lane + p.J - 1;          // dyM[co][m - j] at dc[-j]
    const f32x4* wc = reinterpret_cast<const f32x4*>(ws) + co * p.J * S;
#pragma unroll 2
    for (int j = 0; j < p.J; ++j) {
      const float dv = dc[-j];
#pragma unroll
      for (int r = 0; r < S; ++r) acc[r] += wc[j * S + r] * dv;
    }
  }
  const int m = m0 + lane;
  const int u0 = m * S - p.pad;
  if (u0 >= p.Tin || u0 + S <= 0) return;
  float* dxb = p.y + (long)b * p.y_bs + (long)(g * 4) * p.Tin;
  const bool vec = S == 4 && u0 >= 0 && u0 + 3 < p.Tin && ((u0 | p.Tin) & 3) == 0 && (p.y_bs & 3) == 0 && (((uintptr_t)p.y) & 15) == 0;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    if (vec) {
      if (S == 4) *reinterpret_cast<f32x4*>(dxb + (long)ci * p.Tin + u0) = (f32x4){acc[0][ci], acc[1 % S][ci], acc[2 % S][ci], acc[3 % S][ci]} * p.out_scale;
    } else {
#pragma unroll
      for (int r = 0; r < S; ++r)
        if (u0 + r >= 0 && u0 + r < p.Tin) dxb[(long)ci * p.Tin + u0 + r] = acc[r][ci] * p.out_scale;
    }
  }
}

// ---------------------------------------------------------------------------------------------- weight-grad
// dw[co][ci][k] += sum_{b, t} dyM[co][t] * x[ci][t*s + k - pad];  dbias[co] += sum dyM[co][t].
// grid (G, nsplit): a block owns one group and every nsplit-th sample; thread = weight elements (co, ci, k) in steps of
// 256; the block's partial goes to slab[split] in the module layout, bias partials behind the weights.
__global__ __launch_bounds__(256) void small_group_wgrad_kernel(const SmallGroupP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int g = blockIdx.x, split = blockIdx.y;
  const int XW = p.Tin + 2 * p.pad + p.s;          // padded input row: position q at xs[q + pad]
  float* xs = smem;                                // [4][XW]
  float* ds = xs + 4 * XW;                         // [4][Tout]
  const int nel = 16 * p.K;
  // thread e < 4 K owns the weight elements (co = 0..3, ci, k) of one (ci, k): one x read and one float4 dy read per step
  // for four products (a thread per (co, ci, k) element made the kernel LDS-issue bound)
  const int e_ci = tid / p.K, e_k = tid - e_ci * p.K;
  const bool e_live = tid < 4 * p.K;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;
  // staging roles, the same for every sample: up to 6 input values and 1 dy (+ mask) value per thread
  int xo[6]; bool xk[6];
#pragma unroll
  for (int u = 0; u < 6; ++u) {
    const int i = tid + u * 256;
    const int ci = i / XW, q = i - ci * XW - p.pad;
    xk[u] = i < 4 * XW && q >= 0 && q < p.Tin;
    xo[u] = ci * p.Tin + q;
  }
  const bool dk = tid < 4 * p.Tout;
  float xv[6], dv, mv;
  auto issue = [&](int b) {
    const srd_t xrs = make_srd(p.x + (long)b * p.x_bs + (long)(g * 4) * p.Tin, 4 * p.Tin * 4);
    const srd_t drs = make_srd(p.dy + (long)b * p.dy_bs + (long)(g * 4) * p.Tout, 4 * p.Tout * 4);
    const srd_t mrs = make_srd(p.mask ? p.mask + (long)b * p.mask_bs + (long)(g * 4) * p.Tout : p.dy, p.mask ? 4 * p.Tout * 4 : 0);
#pragma unroll
    for (int u = 0; u < 6; ++u) xv[u] = bload(xrs, xo[u], xk[u]);
    dv = bload(drs, tid, dk);
    mv = bload(mrs, tid, dk);
  };
  issue(split);
  for (int b = split; b < p.B; b += p.nsplit) {
    __syncthreads();                               // the previous sample's tiles are consumed
#pragma unroll
    for (int u = 0; u < 6; ++u) {
      const int i = tid + u * 256;
      if (i < 4 * XW) { float v = xv[u]; if (p.act_in) v = fmaxf(v, v * p.slope_in); xs[i] = v * p.in_scale; }
    }
    if (dk) {                                     // ds layout [t][co]: one float4 per time step
      const float v = dv * p.dy_scale;
      const int co = tid / p.Tout, t = tid - co * p.Tout;
      ds[t * 4 + co] = (!p.mask || mv > 0.f) ? v : v * p.m_slope;
    }
    __syncthreads();
    if (b + p.nsplit < p.B) issue(b + p.nsplit);   // the next sample's loads fly under this sample's products
    if (e_live) {
      const f32x4* dr = reinterpret_cast<const f32x4*>(ds);
      const float* xr = xs + e_ci * XW + e_k;
      f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
      int t = 0;
      for (; t + 1 < p.Tout; t += 2) { s0 += dr[t] * xr[t * p.s]; s1 += dr[t + 1] * xr[(t + 1) * p.s]; }
      if (t < p.Tout) s0 += dr[t] * xr[t * p.s];
      acc += s0 + s1;
    }
    if (tid >= 252) {                              // bias partials on four otherwise idle threads
      float sb = 0.f;
      for (int t = 0; t < p.Tout; ++t) sb += ds[t * 4 + (tid - 252)];
      bacc += sb;
    }
  }
  float* slab = p.slab + (long)split * p.slab_stride;
  if (e_live) {
#pragma unroll
    for (int co = 0; co < 4; ++co) slab[(long)g * nel + (co * 4 + e_ci) * p.K + e_k] = acc[co];
  }
  if (tid >= 252) slab[(long)p.G * nel + g * 4 + (tid - 252)] = bacc;
}

// ============================================================================ 4 -> 16 channels per group: matrix pipe
// Grouped stride-4 Conv1d with 4 input and 16 output channels per group (discriminator layers 1-3: nf -> 4 nf, kernel 41,
// pad 20, nf / 4 groups). Per group the product is 16 x 4K by 4K x T: one full v_mfma_f32_16x16x4_f32 per (tap quad j, input
// channel) (forward) or per (tap quad j, four output channels) (input-grad) and 16 x 16 output tile, nothing padded. A block is ONE wave. It
// owns one group and a run of consecutive 64-column tiles of one sample: the group's weights are read once, coalesced,
// through LDS into registers (4 J per lane) and stay there; per tile the wave stages its
// window in its own LDS, issues the next window's global loads and runs 4 * 4 J MFMAs fed by one ds_read_b32 each.
// No block barrier: the wave's LDS operations execute in order. Loads are dword loads along time (a wave instruction
// covers 256 contiguous bytes); the stores are float4 along time where the rows are 16-byte aligned, float2 where they
// are 8-byte aligned, else scalar.
constexpr int G16_KMAX = 44, G16_JMAX = 11;       // taps; taps per phase
constexpr int G16_NCOL = 64 + G16_JMAX - 1;       // 74: window columns of a 64-column tile, both kernels
// LDS row strides: the two 16-lane halves of a ds_read_b32 32-lane group read neighbouring rows (forward: phase -> phase + 1,
// input-grad: co -> co + 1) and must land on disjoint halves of the 32 banks: 80 = 16 mod 32.
constexpr int G16_XCS = 80, G16_DCS = 80;
// Grid rule. Resident waves: LDS allows 160 KB / 11 KB = 14 one-wave blocks per CU (3.5 per SIMD; the registers allow 4),
// i.e. 256 CUs x 14 = 3584 waves on the chip. A wave walks tpr = ceil(tiles of the launch / 3584) consecutive tiles, so
// that the grid is one resident round where the problem is large enough (the weight load is then paid once per tpr tiles)
// and one tile per wave where it is not; tpr is then evened out over the runs of a row (16 tiles at tpr 5 -> 4 runs of 4).
constexpr int G16_WAVES = 256 * 14;
static inline int g16_tpr(int B, int G, int ntile) {
  long tpr = ((long)B * G * ntile + G16_WAVES - 1) / G16_WAVES;
  tpr = tpr < 1 ? 1 : (tpr > ntile ? ntile : tpr);
  const long nruns = (ntile + tpr - 1) / tpr;
  return (int)((ntile + nruns - 1) / nruns);
}

// Orders the wave's own LDS writes before its later reads (and reads before later writes) for the compiler; the hardware
// executes one wave's LDS operations in order.
__device__ __forceinline__ void g16_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The group's 64 K weights, module layout [co][ci][k], from HBM to ws with coalesced loads (all issued before the first store).
// No predicates: the descriptor ends with the group's block, so elements from 64 K on load as zero, and ws holds 64 * G16_KMAX.
__device__ __forceinline__ void g16_stage_weights(const float* wg, int K, float* ws, int lane) {
  const srd_t wrs = make_srd(wg, 64 * K * 4);
  float wv[G16_KMAX];
#pragma unroll
  for (int i = 0; i < G16_KMAX; ++i) wv[i] = bload(wrs, lane + i * 64, true);
#pragma unroll
  for (int i = 0; i < G16_KMAX; ++i) ws[lane + i * 64] = wv[i];
  g16_wave_sync();
}

// ---------------------------------------------------------------------------------------------- forward
// y[16g+co][t] = bias + sum_{ci, k} W[16g+co][ci][k] * x'[4g+ci][4t + k - pad].  grid (G, B, runs); block = one wave.
// Operands swapped (conv_gemm_kernel's MODE_DOWN form): A = the window, lane (t = lane & 15, phase = lane >> 4); B = the
// weights, lane (co = lane & 15, phase = lane >> 4) holds W[co][ci][4j + phase] for the 4 J steps (j, ci), zero from K on; the
// lane ends with four consecutive steps of output channel co. The steps run j up, ci up with the four phases as the MFMA's
// reduction, the input-grad's j down, cq up: the order of conv_gemm_kernel's main loop (reduced channel = ci * 4 + phase, taps
// outside, four reduced channels per MFMA), so that both kernels return that kernel's bits.
// JT: compile-time J (11); 0 = any J <= 11, one wave-uniform branch per j.
template <int JT>
__global__ __launch_bounds__(64) void group16_fwd_kernel(const SmallGroupP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // 64 * G16_KMAX floats: weights [64][K] first, then the window [ci][phase][G16_XCS]
  const int lane = threadIdx.x, ln = lane & 15, kq = lane >> 4;
  const int g = blockIdx.x, b = blockIdx.y;
  const int ntile = (p.Tout + 63) >> 6;
  const int tile0 = blockIdx.z * p.tpr, tile1 = min(tile0 + p.tpr, ntile);
  const srd_t xrs = make_srd(p.x + (long)b * p.x_bs + (long)(g * 4) * p.Tin, 4 * p.Tin * 4);
  // Window of a tile: positions q0 .. q0 + 295 of the 4 channels, q0 = 256 tile - pad (a multiple of 4). Element (ci, i) of
  // a lane is position q0 + lane + 64 i: phase lane % 4, column lane / 4 + 16 i (i == 4: 40 lanes). One lane-dependent
  // address on either side, the rest are constants. Positions outside [0, Tin) get an out-of-range offset: they load as zero.
  const int lw = (lane & 3) * G16_XCS + (lane >> 2);
  float pre[20];
  auto issue = [&](int tile) {
    const int qb = tile * 256 - p.pad + lane;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int q = qb + 64 * i;
        pre[ci * 5 + i] = bload(xrs, ci * p.Tin + q, (unsigned)q < (unsigned)p.Tin && (i < 4 || lane < 4 * G16_NCOL - 256));
      }
  };
  issue(tile0);                                   // the first window's loads fly under the weight staging
  constexpr int NJ = JT ? JT : G16_JMAX;
  float w[NJ * 4];
  g16_stage_weights(p.w + (long)g * 64 * p.K, p.K, smem, lane);
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int k = 4 * j + kq;
      w[j * 4 + ci] = k < p.K ? smem[(ln * 4 + ci) * p.K + k] : 0.f;
    }
  g16_wave_sync();                                 // the window overwrites the staged weights
  const int ch = g * 16 + ln;
  const float bias = p.bias ? p.bias[ch] : 0.f;
  float* yr = p.y + (long)b * p.y_bs + (long)ch * p.Tout;
  const bool vec4 = (p.Tout & 3) == 0 && (p.y_bs & 3) == 0 && (((uintptr_t)p.y) & 15) == 0;
  const bool vec2 = (p.Tout & 1) == 0 && (p.y_bs & 1) == 0 && (((uintptr_t)p.y) & 7) == 0;
  for (int tile = tile0; tile < tile1; ++tile) {
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int i = 0; i < 5; ++i)
        if (i < 4 || lane < 4 * G16_NCOL - 256) {
          float v = pre[ci * 5 + i];
          if (p.act_in) v = fmaxf(v, v * p.slope_in);
          smem[lw + ci * 4 * G16_XCS + 16 * i] = v * p.in_scale;
        }
    g16_wave_sync();
    if (tile + 1 < tile1) issue(tile + 1);        // the next window's loads fly under this tile's MFMAs
    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Step (j, ci) multiplies W[co][ci][4j + phase] with x'[ci][4 (t + j) + phase], phase = lane >> 4: row ci * 4 + phase, column
    // t + j. The reads run two steps ahead of the MFMAs; the scheduling barrier keeps the compiler from hoisting more of them
    // (the registers hold the weights and the next window). A read ahead past the last step of a short kernel stays inside
    // its row and is not used.
    const float* xb = smem + kq * G16_XCS + ln;
    float xv[3][4];
#pragma unroll
    for (int n = 0; n < 4; ++n) { xv[0][n] = xb[n * 16]; xv[1][n] = xb[4 * G16_XCS + n * 16]; }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (JT || j < p.J) {
#pragma unroll
        for (int s = 4 * j; s < 4 * j + 4; ++s) {
          if (s + 2 < NJ * 4) {
            const float* xk = xb + ((s + 2) & 3) * 4 * G16_XCS + ((s + 2) >> 2);
#pragma unroll
            for (int n = 0; n < 4; ++n) xv[(s + 2) % 3][n] = xk[n * 16];
          }
#pragma unroll
          for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s % 3][n], w[s], acc[n], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    g16_wave_sync();                               // the next window is written after these reads
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int t = tile * 64 + n * 16 + kq * 4;
      if (t >= p.Tout) continue;
      f32x4 v = acc[n] + bias;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = p.post == POST_LRELU ? lrelu_f(v[q], p.post_slope) : v[q];      // no tanh here (host-checked)
      v *= p.out_scale;
      if (vec4) *reinterpret_cast<f32x4*>(yr + t) = v;
      else if (vec2 && t + 3 < p.Tout) {
        *reinterpret_cast<f32x2*>(yr + t) = (f32x2){v[0], v[1]};
        *reinterpret_cast<f32x2*>(yr + t + 2) = (f32x2){v[2], v[3]};
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (t + q < p.Tout) yr[t + q] = v[q];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- input-grad
// dx[4g+ci][4m + r - pad] = sum_{co, j} W[16g+co][ci][r + 4j] * dy'[16g+co][m - j] (zero weight for r + 4j >= K);
// dy' = dy * scale, times lrelu'(mask) with a mask.  grid (G, B, runs); block = one wave; M = (Tin - 1 + pad) / 4 + 1.
// Rows (ci, r), columns m, reduction (j, co) in steps of four output channels: A = the weights, lane (row = lane & 15,
// co % 4 = lane >> 4) holds W[4 cq + lane >> 4][ci][r + 4j] for the 4 J steps (j, cq); B = the dy' window, lane
// (m = lane & 15, co % 4 = lane >> 4). The lane ends with the four phases of (ci = lane >> 4, m): four consecutive input
// positions. JT: compile-time J (11); 0 = any J <= 11, one wave-uniform branch per j.
template <int JT>
__global__ __launch_bounds__(64) void group16_dgrad_kernel(const SmallGroupP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];      // 64 * G16_KMAX floats: weights [64][K] first, then the window [co][G16_DCS]
  const int lane = threadIdx.x, ln = lane & 15, kq = lane >> 4;
  const int g = blockIdx.x, b = blockIdx.y;
  const int M = (p.Tin - 1 + p.pad) / 4 + 1, ntile = (M + 63) >> 6;
  const int tile0 = blockIdx.z * p.tpr, tile1 = min(tile0 + p.tpr, ntile);
  const srd_t drs = make_srd(p.dy + (long)b * p.dy_bs + (long)(g * 16) * p.Tout, 16 * p.Tout * 4);
  const srd_t mrs = make_srd(p.mask ? p.mask + (long)b * p.mask_bs + (long)(g * 16) * p.Tout : p.dy, 16 * p.Tout * 4);
  // Window of a tile: dy' columns m0 - 10 .. m0 + 63 of the 16 channels. A wave instruction covers 32 columns of two
  // channels: element (pr, i) of a lane is channel 2 pr + lane / 32, column lane % 32 + 32 i (i == 2: 10 lanes per half).
  const int rsel = lane >> 5, c = lane & 31;
  const int lw = rsel * G16_DCS + c;
  float pre[24], prm[24];
  auto issue = [&](int tile) {
    const int tb = tile * 64 - (G16_JMAX - 1) + c;
#pragma unroll
    for (int pr = 0; pr < 8; ++pr)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int t = tb + 32 * i, off = (2 * pr + rsel) * p.Tout + t;
        const bool ok = (unsigned)t < (unsigned)p.Tout && (i < 2 || c < G16_NCOL - 64);
        pre[pr * 3 + i] = bload(drs, off, ok);
        prm[pr * 3 + i] = p.mask ? bload(mrs, off, ok) : 1.f;
      }
  };
  issue(tile0);                                   // the first window's loads fly under the weight staging
  constexpr int NJ = JT ? JT : G16_JMAX;
  float w[NJ * 4];
  g16_stage_weights(p.w + (long)g * 64 * p.K, p.K, smem, lane);
  {
    const int ci = ln >> 2, r = ln & 3;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int cq = 0; cq < 4; ++cq) {
        const int k = r + 4 * j;
        w[j * 4 + cq] = k < p.K ? smem[((cq * 4 + kq) * 4 + ci) * p.K + k] : 0.f;
      }
  }
  g16_wave_sync();                                 // the window overwrites the staged weights
  float* dxr = p.y + (long)b * p.y_bs + (long)(g * 4 + kq) * p.Tin;
  const bool vec4 = (p.Tin & 3) == 0 && (p.y_bs & 3) == 0 && (((uintptr_t)p.y) & 15) == 0;
  const bool vec2 = (p.Tin & 1) == 0 && (p.y_bs & 1) == 0 && (((uintptr_t)p.y) & 7) == 0;
  for (int tile = tile0; tile < tile1; ++tile) {
#pragma unroll
    for (int pr = 0; pr < 8; ++pr)
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < 2 || c < G16_NCOL - 64) {
          const float v = pre[pr * 3 + i];      // mask, then scale: the generic prologue's order
          smem[lw + 2 * pr * G16_DCS + 32 * i] = (prm[pr * 3 + i] > 0.f ? v : v * p.m_slope) * p.dy_scale;
        }
    g16_wave_sync();
    if (tile + 1 < tile1) issue(tile + 1);        // the next window's loads fly under this tile's MFMAs
    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Step (j, cq) reads dy'[4 cq + co % 4][m - j]: window column m - m0 + 10 - j. j runs DOWN from J - 1, cq up: conv_gemm_kernel's
    // MODE_UP order. Reads two steps ahead of the MFMAs, as in the forward; slot s of the walk is j = NJ - 1 - s / 4.
    const float* db = smem + kq * G16_DCS + ln + (G16_JMAX - 1);
    auto dptr = [&](int s) { return db + (s & 3) * 4 * G16_DCS - (NJ - 1 - (s >> 2)); };
    // a short kernel (J < NJ) starts at slot s0 = 4 (NJ - J): its read-ahead is primed inside the loop
    float dv[3][4];
#pragma unroll
    for (int s = 0; s < NJ * 4; ++s) {
      const int j = NJ - 1 - (s >> 2);
      if (JT || j < p.J) {
        if ((s & 3) == 0 && (s == 0 || (!JT && j == p.J - 1))) {
#pragma unroll
          for (int n = 0; n < 4; ++n) { dv[s % 3][n] = dptr(s)[n * 16]; dv[(s + 1) % 3][n] = dptr(s + 1)[n * 16]; }
        }
        if (s + 2 < NJ * 4) {
#pragma unroll
          for (int n = 0; n < 4; ++n) dv[(s + 2) % 3][n] = dptr(s + 2)[n * 16];
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j * 4 + (s & 3)], dv[s % 3][n], acc[n], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    g16_wave_sync();                               // the next window is written after these reads
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int u0 = (tile * 64 + n * 16 + ln) * 4 - p.pad;      // a multiple of 4
      if (u0 >= p.Tin || u0 < 0) continue;       // u0 < 0: all four positions are padding (pad % 4 == 0)
      const f32x4 v = acc[n] * p.out_scale;
      if (vec4) *reinterpret_cast<f32x4*>(dxr + u0) = v;
      else if (vec2 && u0 + 3 < p.Tin) {
        *reinterpret_cast<f32x2*>(dxr + u0) = (f32x2){v[0], v[1]};
        *reinterpret_cast<f32x2*>(dxr + u0 + 2) = (f32x2){v[2], v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (u0 + r < p.Tin) dxr[u0 + r] = v[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- host
static inline int sg_cs(int s, int K) { return ((64 + (K + s - 1) / s + 1 + 15) / 16) * 16; }

hipError_t launch_small_group_fwd(SmallGroupP p, hipStream_t st) {
  p.J = (p.K + p.s - 1) / p.s;
  p.CS = sg_cs(p.s, p.K);
  const size_t lds = (size_t)4 * (4 * p.s * p.CS + 16 * p.K) * sizeof(float);
  if (lds > 64 * 1024 || 16 * p.K > 768) return hipErrorNotSupported;
  const dim3 grid((p.G + 3) / 4, p.B, (p.Tout + 63) / 64);
  if (p.s == 2) { TDVC_TRACE(small_group_fwd_kernel<2>); hipLaunchKernelGGL(small_group_fwd_kernel<2>, grid, dim3(256), lds, st, p); }
  else if (p.s == 4) { TDVC_TRACE(small_group_fwd_kernel<4>); hipLaunchKernelGGL(small_group_fwd_kernel<4>, grid, dim3(256), lds, st, p); }
  else if (p.s == 8) { TDVC_TRACE(small_group_fwd_kernel<8>); hipLaunchKernelGGL(small_group_fwd_kernel<8>, grid, dim3(256), lds, st, p); }
  else return hipErrorNotSupported;
  return hipGetLastError();
}

hipError_t launch_small_group_dgrad(SmallGroupP p, hipStream_t st) {
  p.J = (p.K + p.s - 1) / p.s;
  if (p.s > 8 || 16 * p.J * p.s > 768 || p.J > 64) return hipErrorNotSupported;
  const size_t lds = (size_t)4 * (4 * (64 + p.J) + 16 * p.J * p.s) * sizeof(float);
  if (lds > 64 * 1024) return hipErrorNotSupported;
  const int M = (p.Tin - 1 + p.pad) / p.s + 1;
  const dim3 grid((p.G + 3) / 4, p.B, (M + 63) / 64);
  if (p.s == 2) { TDVC_TRACE(small_group_dgrad_kernel<2>); hipLaunchKernelGGL(small_group_dgrad_kernel<2>, grid, dim3(256), lds, st, p); }
  else if (p.s == 4) { TDVC_TRACE(small_group_dgrad_kernel<4>); hipLaunchKernelGGL(small_group_dgrad_kernel<4>, grid, dim3(256), lds, st, p); }
  else if (p.s == 8) { TDVC_TRACE(small_group_dgrad_kernel<8>); hipLaunchKernelGGL(small_group_dgrad_kernel<8>, grid, dim3(256), lds, st, p); }
  else return hipErrorNotSupported;
  return hipGetLastError();
}

// 4 -> 16 channels per group, stride 4 (the caller has checked the channel counts). Declines what the kernels do not cover.
static bool group16_launchable(const SmallGroupP& p) {
  return p.s == 4 && p.K >= 1 && p.K <= G16_KMAX && p.pad >= 0 && (p.pad & 3) == 0 && p.B <= 65535 && p.G >= 1;
}
static constexpr size_t G16_LDS = (size_t)64 * G16_KMAX * sizeof(float);      // the staged weights; the windows (16 rows of 80) are smaller

hipError_t launch_group16_fwd(SmallGroupP p, hipStream_t st) {
  if (!group16_launchable(p) || p.post == POST_TANH) return hipErrorNotSupported;
  p.J = (p.K + 3) / 4;
  const int ntile = (p.Tout + 63) / 64;
  p.tpr = g16_tpr(p.B, p.G, ntile);
  const dim3 grid(p.G, p.B, (ntile + p.tpr - 1) / p.tpr);
  if (grid.z > 65535) return hipErrorNotSupported;
  const size_t lds = G16_LDS;
  if (p.J == G16_JMAX) { TDVC_TRACE(group16_fwd_kernel<G16_JMAX>); hipLaunchKernelGGL(group16_fwd_kernel<G16_JMAX>, grid, dim3(64), lds, st, p); }
  else { TDVC_TRACE(group16_fwd_kernel<0>); hipLaunchKernelGGL(group16_fwd_kernel<0>, grid, dim3(64), lds, st, p); }
  return hipGetLastError();
}

hipError_t launch_group16_dgrad(SmallGroupP p, hipStream_t st) {
  if (!group16_launchable(p)) return hipErrorNotSupported;
  p.J = (p.K + 3) / 4;
  const int M = (p.Tin - 1 + p.pad) / 4 + 1, ntile = (M + 63) / 64;
  p.tpr = g16_tpr(p.B, p.G, ntile);
  const dim3 grid(p.G, p.B, (ntile + p.tpr - 1) / p.tpr);
  if (grid.z > 65535) return hipErrorNotSupported;
  const size_t lds = G16_LDS;
  if (p.J == G16_JMAX) { TDVC_TRACE(group16_dgrad_kernel<G16_JMAX>); hipLaunchKernelGGL(group16_dgrad_kernel<G16_JMAX>, grid, dim3(64), lds, st, p); }
  else { TDVC_TRACE(group16_dgrad_kernel<0>); hipLaunchKernelGGL(group16_dgrad_kernel<0>, grid, dim3(64), lds, st, p); }
  return hipGetLastError();
}

size_t small_group_wgrad_workspace(int B, int G, int K) {
  const int nsplit = B >= 8 ? 4 : 1;
  return (size_t)nsplit * ((size_t)G * 16 * K + (size_t)G * 4) * sizeof(float);
}

hipError_t launch_small_group_wgrad(SmallGroupP p, float* dw, float* dbias, void* workspace, size_t workspace_bytes, hipStream_t st) {
  if (4 * p.K > 252 || 4 * (p.Tin + 2 * p.pad + p.s) > 6 * 256 || 4 * p.Tout > 256) return hipErrorNotSupported;
  p.nsplit = p.B >= 8 ? 4 : 1;
  const long nW = (long)p.G * 16 * p.K, n = nW + (long)p.G * 4;
  if (workspace_bytes < (size_t)p.nsplit * n * sizeof(float) || !workspace) return hipErrorNotSupported;
  const size_t lds = (size_t)(4 * (p.Tin + 2 * p.pad + p.s) + 4 * p.Tout) * sizeof(float);
  if (lds > 64 * 1024) return hipErrorNotSupported;
  p.slab = (float*)workspace; p.slab_stride = n;
  TDVC_TRACE(small_group_wgrad_kernel);
  hipLaunchKernelGGL(small_group_wgrad_kernel, dim3(p.G, p.nsplit), dim3(256), lds, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // bias partials ride behind the weights; without a bias gradient only the weights are folded
  return launch_slab_reduce(p.slab, p.nsplit, n, dbias ? n : nW, dw, (int)nW, nW, st, nW, dbias);
}

}  // namespace tdvc
