// The split-bf16 "x6" scheme, shared by its kernels (conv_fwd_x6.hip, conv_wgrad_x6.hip): fp32-accurate products on the bf16 matrix
// pipe. Every fp32 operand is cut EXACTLY into three bf16 pieces (x = hi + mid + lo: 3 x 8 significant bits, by truncation, no
// rounding anywhere) and the product is the six piece products whose weight is >= 2^-16 of the leading one,
//     a*b ~= lo.hi + hi.lo + mid.mid + mid.hi + hi.mid + hi.hi      (dropped: mid.lo, lo.mid, lo.lo <= 2^-24 relative)
// each an exact bf16 x bf16 product accumulated in fp32 by v_mfma_f32_16x16x32_bf16.
#pragma once

namespace tdvc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int X6_RS = 32;               // bf16 row length of every LDS image: 64 B = one k-block of 32, no padding (x6_swz)

// exact: f = h + m + l, each piece the UPPER half of its word (l's lower half is zero by construction: 24 significant bits in all;
// it is left unmasked and dropped by the pack). f must be a scalar VARIABLE (hipcc 7.2: __builtin_bit_cast applied DIRECTLY to a
// vector element expression reads element 0 for every index)
__device__ __forceinline__ void x6_split(const float f, unsigned& h, unsigned& m, unsigned& l) {
  h = __builtin_bit_cast(unsigned, f) & 0xffff0000u;
  const float r1 = f - __builtin_bit_cast(float, h);
  m = __builtin_bit_cast(unsigned, r1) & 0xffff0000u;
  const float r2 = r1 - __builtin_bit_cast(float, m);
  l = __builtin_bit_cast(unsigned, r2);
}
__device__ __forceinline__ unsigned x6_pack_hi(unsigned a, unsigned b) {   // {upper half of a, upper half of b}: a in the low 16 bits
  return __builtin_amdgcn_perm(b, a, 0x07060302u);
}
// the split of 4 values, packed 4 x 16 bit per piece (element q in bits 16q .. 16q + 15)
__device__ __forceinline__ void x6_split4(const f32x4 v, u32x2& hi, u32x2& mid, u32x2& lo) {
  unsigned h[4], m[4], l[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float f = v[q];
    x6_split(f, h[q], m[q], l[q]);
  }
  hi = (u32x2){x6_pack_hi(h[0], h[1]), x6_pack_hi(h[2], h[3])};
  mid = (u32x2){x6_pack_hi(m[0], m[1]), x6_pack_hi(m[2], m[3])};
  lo = (u32x2){x6_pack_hi(l[0], l[1]), x6_pack_hi(l[2], l[3])};
}

// LDS element offset of slot q (8 bf16) of row r: the 16-byte slot q of row r lives at slot q ^ ((r >> 1) & 3). ds_read_b128 serves a
// wave in four NON-contiguous 16-lane groups ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md, LDS), so a group mixes rows of two
// k-quarters: padded 80-byte rows made every group 2-way conflicting (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.50 forward, 0.49
// weight-grad in profiles/r03_pmc.txt). With this XOR any 16 consecutive rows read by lanes (row = base + (lane & 15), q = lane >> 4)
// touch 16 distinct 4-bank slots in every group, for every base (tools/lds_swizzle_check.py); planes are multiples of 8 rows.
__device__ __forceinline__ int x6_swz(int r, int q) { return r * X6_RS + 8 * (q ^ ((r >> 1) & 3)); }

// The three pieces of one position -> the three planes (stride `plane` elements) of an LDS or global image. V: u32x2 (4 values) or
// unsigned short (one, the upper half of its word already shifted down).
template <class V>
__device__ __forceinline__ void x6_store3(unsigned short* img, int plane, int off, V h, V m, V l) {
  *reinterpret_cast<V*>(img + 0 * plane + off) = h;
  *reinterpret_cast<V*>(img + 1 * plane + off) = m;
  *reinterpret_cast<V*>(img + 2 * plane + off) = l;
}
__device__ __forceinline__ void x6_split_store4(unsigned short* img, int plane, int off, const f32x4 v) {
  u32x2 h, m, l;
  x6_split4(v, h, m, l);
  x6_store3(img, plane, off, h, m, l);
}
__device__ __forceinline__ bf16x8 x6_frag(const unsigned short* img, int off) {       // one ds_read_b128 fragment of 8 k values
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + off));
}

// One k-block of the product, pieces [0] = hi, [1] = mid, [2] = lo. The ORDER is the numerical contract: smallest products first.
__device__ __forceinline__ void x6_mfma(f32x4& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  f32x4 c = acc;
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
  acc = c;
}

}  // namespace tdvc
