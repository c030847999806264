// The CREPE pitch tracker (torchcrepe's `tiny` and `full` networks, the reference's util/crepe.py filtered_pitch), restated in
// include/tdvc.h: the framing front end, the six conv blocks, the classifier head and the per-frame decoders. The forward; the backward
// with respect to the signal is pitch_crepe_bwd.hip, which needs tdvc_crepe_conv_train here: the conv launch that also writes the pooling
// decision of every output (one kernel template, a compile-time switch, the same instructions for y).
//
// tdvc_crepe_frames  a block per frame: 1024 samples around f hop (the row zero-padded by 512 on both sides, samples at and past the
//                    row's length never read), mean and unbiased standard deviation in float64 (two passes, pairwise combine of the
//                    four waves), (x - mean) / max(1e-10, std) rounded once at the store
// tdvc_crepe_conv    one launch per layer: conv + bias + ReLU + folded BatchNorm + max-pool 2, below
// tdvc_crepe_head    the position-major flatten, Linear(., 360) and the sigmoid: a wave per (output, 8 frames), float64 sums
// tdvc_crepe_decode  a thread per frame: mask, argmax or weighted argmax (or the caller's bins), periodicity, cents -> Hz in float64,
//                    threshold; or the in-range log-softmax lattice for tdvc_viterbi_path
//
// The conv kernel. An implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32): M = 16 output channels, the columns are (frame, conv
// position) pairs, the reduction runs over (input channel, tap). A workgroup of 256 threads owns 16 output channels x 256 columns,
// i.e. 256 / LC whole frames of LC conv positions (LC = 256 for layer 1, 128 .. 8 for layers 2 .. 6): frames are independent (each
// is zero-padded on its own), so a block never needs a neighbour's samples. Wave w owns the columns [64 w, 64 w + 64) as four 16 x 16
// accumulator tiles: four independent MFMA chains per A operand. The four k of one MFMA are four consecutive TAPS (lane group q =
// lane / 16 is tap 4 kk + q), which serves both geometries with one loop:
//   K = 64, stride 1:  chunk = 2 input channels x 64 taps; xs[channel][frame][LC + 64] holds the frame behind 31 zeros and in front
//                      of 32; lane (j, q) reads xs[.. + pos_j + 4 kk + q]: 17 consecutive words per 32-lane half, no bank conflict
//   K = 512, stride 4: chunk = 128 taps of the one input channel; the padded frame is staged as four PHASE planes, plane q holds
//                      x[4 m + q + k0 - 254], so that position p and tap 4 kk + q meet at plane q, word p + kk: consecutive words
//                      again instead of a stride of 4 (which would be a 2-way conflict); planes are 304 = 16 mod 32 words apart, so
//                      q = 0 and q = 1 of one half fall into disjoint halves of the 32 banks
// Weights of a chunk are ws[16][130] (130 = 2 mod 32: lane (j, q) reads bank 2 j + q). The next chunk is loaded into registers
// before the MFMAs of the current one and stored to LDS behind them. Each chunk (128 products per chain) is summed from zero and then
// added to the running sum: layer 2 of `tiny` reduces over 8192 products, and this keeps its rounding at that of a blocked summation.
// Epilogue: + bias, ReLU, v scale + shift (the BatchNorm comes AFTER the ReLU and its scale may be negative, so the pool cannot move
// in front of the affine), then the max over the position pair, which sits in neighbouring lanes (one __shfl_xor), stored by the
// even lane. No atomics, one fixed order: bit-identical from call to call, and a frame's result does not depend on its batch.
#include <math.h>

#include "../../include/tdvc.h"
#include "api_util.h"
#include "pitch_crepe.h"
#include "reduce.h"

namespace tdvc {

constexpr int CR_PL = 304;           // phase plane pitch of the stride-4 geometry: 256 + 32 words used
constexpr double CR_CENTS0 = 1997.3794084376191;

// ----------------------------------------------------------------------------------------------------------------- frames
__global__ __launch_bounds__(256) void crepe_frames_kernel(const float* x, long x_bs, const int* lengths, int T, int hop, int F, float* out) {
  __shared__ double red[4];
  const int t = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  const int n = row_len(lengths, b, T);
  float* o = out + ((long)b * F + f) * CR_WIN;
  if (f >= 1 + n / hop) {                                                   // uniform: past the row's own frame count
#pragma unroll
    for (int k = 0; k < 4; ++k) o[t + 256 * k] = 0.f;
    return;
  }
  const float* row = x + b * x_bs;
  const long q0 = (long)f * hop - CR_WIN / 2;
  double v[4], s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long q = q0 + t + 256 * k;
    v[k] = q >= 0 && q < n ? (double)row[q] : 0.0;
    s += v[k];
  }
  const double mean = block_sum_pairwise(s, red, t) / (double)CR_WIN;
  __syncthreads();                                                          // red is written again below
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[k] -= mean; ss = fma(v[k], v[k], ss); }
  const double sd = sqrt(block_sum_pairwise(ss, red, t) / (double)(CR_WIN - 1));
  const double den = fmax(1e-10, sd);
#pragma unroll
  for (int k = 0; k < 4; ++k) o[t + 256 * k] = (float)(v[k] / den);
}

// ------------------------------------------------------------------------------------------------------------------- conv
struct CrConvP {
  int N, Cin, Cout;
  const float* x; const float* w; const float* bias; const float* scale; const float* shift;
  float* y;
  unsigned char* code;                                           // TRAIN only: [N][Cout][LC / 2]
};

// S = 4: Cin = 1, K = 512, 1024 samples in, LC = 256 conv positions. S = 1: K = 64, LC positions in and out.
// TRAIN: also the pooling decision of every output (tdvc_crepe_conv_train); y is computed by the same instructions either way.
template <int S, int LC, bool TRAIN>
__global__ __launch_bounds__(CR_THREADS, 2) void crepe_conv_kernel(CrConvP p) {
  constexpr int FPB = 256 / LC;                                  // frames per block
  constexpr int CH = S == 4 ? 1 : 2;                             // input channels per chunk
  constexpr int K = S == 4 ? 512 : 64;
  constexpr int LIN = S == 4 ? CR_WIN : LC;
  constexpr int PADL = S == 4 ? 254 : 31;
  constexpr int LP = LC + 64;                                    // S = 1: words per (channel, frame)
  constexpr int XC = S == 4 ? 4 * CR_PL : FPB * LP;              // words per channel
  constexpr int XTOT = CH * XC;
  constexpr int XS = (XTOT + CR_THREADS - 1) / CR_THREADS;
  constexpr int NW = 16 * CR_KCH / 4 / CR_THREADS;               // float4 of weights per thread: 2
  static_assert(S == 4 ? LC == 256 : (LC >= 8 && LC <= 128 && 256 % LC == 0), "geometry");
  static_assert(S == 4 || XTOT % CR_THREADS == 0, "staging shape");
  __shared__ float xs[XTOT];
  __shared__ float ws[16 * CR_WP];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, j = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * FPB, co0 = blockIdx.y * 16;
  const int R = p.Cin * K;                                       // the reduction's length, a multiple of CR_KCH
  // what this thread stages per chunk: XS words of xs (their source does not depend on the chunk up to a constant) and NW float4 of weights
  int src[XS];
#pragma unroll
  for (int sl = 0; sl < XS; ++sl) {
    const int e = t + CR_THREADS * sl;
    if constexpr (S == 4) {
      const int pl = e / CR_PL, m = e - pl * CR_PL;
      src[sl] = e < XTOT && m < 288 && n0 < p.N ? 4 * m + pl - PADL : -(1 << 20);     // + k0: the sample of the frame; out of [0, 1024): a zero
    } else {
      const int cl = e / XC, r = e - cl * XC, fl = r / LP, i = r - fl * LP;
      const int s = i - PADL;
      src[sl] = s >= 0 && s < LC && n0 + fl < p.N ? ((n0 + fl) * p.Cin + cl) * LIN + s : -1;   // + c0 LIN; N Cin LIN < 2^31 (checked on the host)
    }
  }
  const float* wsrc[NW];
#pragma unroll
  for (int sl = 0; sl < NW; ++sl) {
    const int u = t + CR_THREADS * sl, r = u / (CR_KCH / 4);
    wsrc[sl] = p.w + (long)(co0 + r) * R + 4 * (u - r * (CR_KCH / 4));
  }
  float xreg[XS];
  float4 wreg[NW];
  auto load = [&](int ch) {                                                 // chunk ch: products [128 ch, 128 ch + 128) of the reduction
#pragma unroll
    for (int sl = 0; sl < XS; ++sl) {
      float v = 0.f;
      if constexpr (S == 4) {
        const int s = src[sl] + ch * CR_KCH;
        if (s >= 0 && s < LIN) v = p.x[(long)n0 * LIN + s];
      } else {
        if (src[sl] >= 0) v = p.x[src[sl] + ch * CH * LIN];
      }
      xreg[sl] = v;
    }
#pragma unroll
    for (int sl = 0; sl < NW; ++sl) wreg[sl] = *reinterpret_cast<const float4*>(wsrc[sl] + ch * CR_KCH);
  };
  // the column of this lane in accumulator tile nt, as a word offset into one channel of xs
  int coloff[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = 64 * wv + 16 * nt + j;
    coloff[nt] = S == 4 ? q * CR_PL + col : (col / LC) * LP + (col % LC) + q;
  }
  cr_f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = cr_f32x4{0.f, 0.f, 0.f, 0.f};
  const int nch = R / CR_KCH;
  load(0);
  for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
    for (int sl = 0; sl < XS; ++sl)
      if (S != 4 || t + CR_THREADS * sl < XTOT) xs[t + CR_THREADS * sl] = xreg[sl];
#pragma unroll
    for (int sl = 0; sl < NW; ++sl) {
      const int u = t + CR_THREADS * sl, r = u / (CR_KCH / 4);
      float* d = ws + r * CR_WP + 4 * (u - r * (CR_KCH / 4));
      d[0] = wreg[sl].x; d[1] = wreg[sl].y; d[2] = wreg[sl].z; d[3] = wreg[sl].w;
    }
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1);
    cr_f32x4 part[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) part[nt] = cr_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < CR_KCH / 4; ++kk) {
      const float a = ws[j * CR_WP + 4 * kk + q];
      // S = 4: plane q, word pos + kk. S = 1: product 4 kk + q is channel kk / 16 of the chunk, tap 4 (kk % 16) + q
      const int step = S == 4 ? kk : (kk / (K / 4)) * XC + 4 * (kk % (K / 4));
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        part[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xs[coloff[nt] + step], part[nt], 0, 0, 0);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] += part[nt];
    __syncthreads();
  }
  constexpr int LOUT = LC / 2;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int co = co0 + 4 * q + r;
    const float bi = p.bias[co], sc = p.scale[co], sh = p.shift[co];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int col = 64 * wv + 16 * nt + j, n = n0 + col / LC, pos = col % LC;
      const float z = acc[nt][r] + bi;
      const float v = fmaf(fmaxf(z, 0.f), sc, sh);
      const float vo = __shfl_xor(v, 1);                                    // the other position of the pair: the neighbouring lane
      const float m = fmaxf(v, vo);
      const long at = ((long)n * p.Cout + co) * LOUT + (pos >> 1);
      if constexpr (TRAIN) {                                                // the odd position wins only if it is strictly larger
        const float zo = __shfl_xor(z, 1);
        const bool odd = vo > v;
        const unsigned char cd = (odd ? zo : z) <= 0.f ? CR_CODE_DEAD : (odd ? CR_CODE_ODD : CR_CODE_EVEN);
        if (!(j & 1) && n < p.N) p.code[at] = cd;
      }
      if (!(j & 1) && n < p.N) p.y[at] = m;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- head
// x [N][C][P] (the last conv block's output), w [O][P C] over the position-major flatten (feature l C + c is x[n][c][l]);
// act[n / F][o][n % F] = sigmoid(w[o] . flat(x[n]) + bias[o]). A wave per (o, 8 frames): a weight is read once for eight frames.
constexpr int CR_HF = 8;
__global__ __launch_bounds__(256) void crepe_head_kernel(const float* x, const float* w, const float* bias, int N, int C, int P, int O, int F,
                                                         float* act) {
  const int lane = threadIdx.x & 63, o = blockIdx.y * 4 + (threadIdx.x >> 6), n0 = blockIdx.x * CR_HF;
  const int PC = P * C;
  const float* wr = w + (long)o * PC;
  double acc[CR_HF];
#pragma unroll
  for (int fr = 0; fr < CR_HF; ++fr) acc[fr] = 0.0;
  for (int i = lane; i < PC; i += 64) {
    const int l = i / C, c = i - l * C;
    const double wi = (double)wr[i];
    const float* xp = x + (long)n0 * PC + c * P + l;
#pragma unroll
    for (int fr = 0; fr < CR_HF; ++fr)
      if (n0 + fr < N) acc[fr] = fma(wi, (double)xp[(long)fr * PC], acc[fr]);
  }
#pragma unroll
  for (int fr = 0; fr < CR_HF; ++fr) {
    const double z = wave_sum(acc[fr]) + (double)bias[o];
    const int n = n0 + fr;
    if (lane == 0 && n < N) act[((long)(n / F) * O + o) * F + n % F] = (float)(1.0 / (1.0 + exp(-z)));
  }
}

// ----------------------------------------------------------------------------------------------------------------- decode
struct CrDecP {
  const float* act; long a_bs, a_cs;
  int B, F, nbins, lo, hi, mode; float threshold;
  const int* frames; const int* bins;
  float* pitch; float* periodicity; float* lattice;
};

__global__ __launch_bounds__(64) void crepe_decode_kernel(CrDecP p) {
  const int f = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (f >= p.F) return;
  const float* a = p.act + b * p.a_bs + f;
  if (p.mode == TDVC_CREPE_LATTICE) {                                       // log-softmax over the in-range bins
    double mx = -INFINITY;
    for (int k = p.lo; k < p.hi; ++k) mx = fmax(mx, (double)a[k * p.a_cs]);
    double s = 0.0;
    for (int k = p.lo; k < p.hi; ++k) s += exp((double)a[k * p.a_cs] - mx);
    const double lse = mx + log(s);
    float* o = p.lattice + ((long)b * p.F + f) * (p.hi - p.lo);
    for (int k = p.lo; k < p.hi; ++k) o[k - p.lo] = (float)((double)a[k * p.a_cs] - lse);
    return;
  }
  const long at = (long)b * p.F + f;
  if (f >= row_len(p.frames, b, p.F)) { p.pitch[at] = 0.f; p.periodicity[at] = 0.f; return; }
  int best;
  if (p.bins) {
    best = min(max(p.bins[at], p.lo), p.hi - 1);
  } else {
    best = p.lo;
    float bv = a[p.lo * p.a_cs];
    for (int k = p.lo + 1; k < p.hi; ++k) {
      const float v = a[k * p.a_cs];
      if (v > bv) { bv = v; best = k; }                                     // strict: the lowest index among equal maxima
    }
  }
  const float per = a[best * p.a_cs];
  double cents = 20.0 * best + CR_CENTS0;
  if (p.mode == TDVC_CREPE_WEIGHTED) {
    const int k0 = max(max(0, best - 4), p.lo), k1 = min(min(p.nbins, best + 5), p.hi);     // the window, cut by 0, nbins and the mask
    double sw = 0.0, swc = 0.0;
    for (int k = k0; k < k1; ++k) {
      const double wk = 1.0 / (1.0 + exp(-(double)a[k * p.a_cs]));          // torchcrepe's second sigmoid, kept
      sw += wk;
      swc = fma(wk, 20.0 * k + CR_CENTS0, swc);
    }
    cents = swc / sw;
  }
  p.periodicity[at] = per;
  p.pitch[at] = per < p.threshold ? 0.f : (float)(10.0 * exp2(cents / 1200.0));
}

template <int S, int LC>
static void crepe_conv_launch(const CrConvP& p, hipStream_t st) {
  constexpr int FPB = 256 / LC;
  const dim3 grid((p.N + FPB - 1) / FPB, p.Cout / 16);
  if (p.code) hipLaunchKernelGGL((crepe_conv_kernel<S, LC, true>), grid, dim3(CR_THREADS), 0, st, p);
  else hipLaunchKernelGGL((crepe_conv_kernel<S, LC, false>), grid, dim3(CR_THREADS), 0, st, p);
}

// the checks and the launch of tdvc_crepe_conv and tdvc_crepe_conv_train: code == nullptr is the plain forward
static int crepe_conv_run(const tdvc_crepe_conv_args* a, unsigned char* code, bool train, void* stream);

}  // namespace tdvc

extern "C" int tdvc_crepe_frames(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, int32_t hop, int32_t F,
                                 float* frames, void* stream) {
  using namespace tdvc;
  if (B < 0 || T < 0 || s_bs < 0) return tdvc_fail(TDVC_EINVAL, "crepe_frames: negative B, T or stride");
  if (hop < 1) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames: hop must be at least 1");
  if (T < 1) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames: rows with no sample");
  if (B > 65535 || T > (1 << 28)) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_frames: B > 65535 or T > 2^28");
  if (F != 1 + T / hop) return tdvc_fail(TDVC_EINVAL, "crepe_frames: F must be 1 + T / hop");
  if (B == 0) return TDVC_OK;
  if (!signal || !frames) return tdvc_fail(TDVC_EINVAL, "crepe_frames: null pointer");
  hipLaunchKernelGGL(crepe_frames_kernel, dim3(F, B), dim3(256), 0, (hipStream_t)stream, signal, (long)s_bs, lengths, T, hop, F, frames);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_crepe_conv(const tdvc_crepe_conv_args* a, void* stream) { return tdvc::crepe_conv_run(a, nullptr, false, stream); }

extern "C" int tdvc_crepe_conv_train(const tdvc_crepe_conv_args* a, uint8_t* code, void* stream) { return tdvc::crepe_conv_run(a, code, true, stream); }

static int tdvc::crepe_conv_run(const tdvc_crepe_conv_args* a, unsigned char* code, bool train, void* stream) {
  if (!a) return tdvc_fail(TDVC_EINVAL, "crepe_conv: null arguments");
  if (a->N < 0 || a->Cin < 1 || a->Cout < 1) return tdvc_fail(TDVC_EINVAL, "crepe_conv: negative N or a channel count below 1");
  const bool first = a->stride == 4 && a->K == 512 && a->Cin == 1 && a->Lin == CR_WIN;
  const bool later = a->stride == 1 && a->K == 64 && (a->Lin == 128 || a->Lin == 64 || a->Lin == 32 || a->Lin == 16 || a->Lin == 8);
  if (!first && !later)
    return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_conv: the geometry must be Cin 1, K 512, stride 4 on 1024 samples, or K 64, stride 1 on 128, 64, 32, 16 or 8 positions");
  if (a->Cout % 16 || (later && a->Cin % 16)) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_conv: channel counts must be multiples of 16");
  const int lc = first ? 256 : a->Lin;
  if (a->Cout > (1 << 16) || (double)a->N * a->Cin * a->Lin > 2147483647.0 || (double)a->N * a->Cout * (lc / 2) > 2147483647.0 || a->N > (1 << 22))
    return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_conv: more than 2^16 output channels, 2^22 frames or 2^31 elements");
  if (a->N == 0) return TDVC_OK;
  if (!a->x || !a->w || !a->bias || !a->scale || !a->shift || !a->y || (train && !code)) return tdvc_fail(TDVC_EINVAL, "crepe_conv: null pointer");
  if (((uintptr_t)a->w & 15) != 0) return tdvc_fail(TDVC_EINVAL, "crepe_conv: weights must be 16-byte aligned");
  CrConvP p;
  p.N = a->N; p.Cin = a->Cin; p.Cout = a->Cout; p.x = a->x; p.w = a->w; p.bias = a->bias; p.scale = a->scale; p.shift = a->shift; p.y = a->y; p.code = code;
  hipStream_t st = (hipStream_t)stream;
  if (first) crepe_conv_launch<4, 256>(p, st);
  else if (lc == 128) crepe_conv_launch<1, 128>(p, st);
  else if (lc == 64) crepe_conv_launch<1, 64>(p, st);
  else if (lc == 32) crepe_conv_launch<1, 32>(p, st);
  else if (lc == 16) crepe_conv_launch<1, 16>(p, st);
  else crepe_conv_launch<1, 8>(p, st);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_crepe_head(const float* x, int32_t N, int32_t C, int32_t P, const float* w, const float* bias, int32_t O, int32_t F,
                               float* act, void* stream) {
  using namespace tdvc;
  if (N < 0 || C < 1 || P < 1 || O < 1 || F < 1) return tdvc_fail(TDVC_EINVAL, "crepe_head: negative N, or C, P, O or F below 1");
  if (C % 16 || O % 4) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_head: C must be a multiple of 16 and the output count of 4");
  if (N % F) return tdvc_fail(TDVC_EINVAL, "crepe_head: N must be a multiple of the frames per row F");
  if (O > (1 << 16) || N > (1 << 22) || (double)N * C * P > 2147483647.0 || (double)C * P > (1 << 24))
    return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_head: more than 2^16 outputs, 2^22 frames, 2^24 features or 2^31 elements");
  if (N == 0) return TDVC_OK;
  if (!x || !w || !bias || !act) return tdvc_fail(TDVC_EINVAL, "crepe_head: null pointer");
  hipLaunchKernelGGL(crepe_head_kernel, dim3((N + CR_HF - 1) / CR_HF, O / 4), dim3(256), 0, (hipStream_t)stream, x, w, bias, N, C, P, O, F, act);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}

extern "C" int tdvc_crepe_decode(const float* act, int64_t a_bs, int64_t a_cs, int32_t B, int32_t F, int32_t n_bins, int32_t lo, int32_t hi,
                                 int32_t mode, float threshold, const int32_t* frames, const int32_t* bins, float* pitch, float* periodicity,
                                 float* lattice, void* stream) {
  using namespace tdvc;
  if (B < 0 || F < 0 || n_bins < 1 || a_bs < 0 || a_cs < 0) return tdvc_fail(TDVC_EINVAL, "crepe_decode: negative size or stride");
  if (mode != TDVC_CREPE_ARGMAX && mode != TDVC_CREPE_WEIGHTED && mode != TDVC_CREPE_LATTICE)
    return tdvc_fail(TDVC_EINVAL, "crepe_decode: mode must be 0 (argmax), 1 (weighted argmax) or 2 (lattice)");
  if (lo < 0 || hi > n_bins || lo >= hi) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_decode: the bin range [lo, hi) is empty or leaves [0, n_bins)");
  if (F > 0 && a_cs < F) return tdvc_fail(TDVC_EINVAL, "crepe_decode: bin stride below F");
  if (B > 65535 || F > (1 << 24) || n_bins > 4096) return tdvc_fail(TDVC_EUNSUPPORTED, "crepe_decode: B > 65535, F > 2^24 or more than 4096 bins");
  if (bins && mode != TDVC_CREPE_ARGMAX) return tdvc_fail(TDVC_EINVAL, "crepe_decode: given bins go with mode 0");
  if (B == 0 || F == 0) return TDVC_OK;
  if (!act || (mode == TDVC_CREPE_LATTICE ? !lattice : (!pitch || !periodicity))) return tdvc_fail(TDVC_EINVAL, "crepe_decode: null pointer");
  CrDecP p;
  p.act = act; p.a_bs = a_bs; p.a_cs = a_cs; p.B = B; p.F = F; p.nbins = n_bins; p.lo = lo; p.hi = hi; p.mode = mode; p.threshold = threshold;
  p.frames = frames; p.bins = bins; p.pitch = pitch; p.periodicity = periodicity; p.lattice = lattice;
  hipLaunchKernelGGL(crepe_decode_kernel, dim3((F + 63) / 64, B), dim3(64), 0, (hipStream_t)stream, p);
  TDVC_CHECK_LAUNCH();
  return TDVC_OK;
}
