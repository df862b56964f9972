// The dense 16-bit convolution tile shared by bev_conv.hip, cam_neck.hip, cam_nets.hip, res_block.hip, bottleneck.hip and
// resnet_stem.hip: device helpers only, no kernels and no state.
//
// The shared formulation: an implicit GEMM D[channel][pixel] = W[channel][(chunk, tap, ci)] * X[(chunk, tap, ci)][pixel] on
// v_mfma_f32_16x16x32_{f16,bf16} with fp32 accumulation.
//   * A (weights): packed on the host in fragment order, [channel tile of 16][chunk][tap][64 lanes][8]; one 16-byte load per lane
//     and MFMA, streaming from L2.
//   * B (input): a tile of pixels is staged in LDS in chunks of CK = 32 channels as [pixel][PSTR]; a lane's fragment, the 8 channels
//     8 (lane >> 4) .. of pixel lane & 15 of a row of 16, is one 16-byte LDS read, and all taps read the same chunk from shifted
//     addresses.  Staging moves UNITS: 8 channels of one pixel, 16 bytes, one load from NHWC or eight 2-byte loads from NCHW.
//     Cells outside the map and channels past the last are zero in LDS; no address outside a tensor is formed.
//   * D: pixel on the lane (lane & 15), channel = 16 tile + 4 (lane >> 4) + reg.  Four channels of one pixel go through
//     y = fma(acc, scale, shift) in fp32, the caller's residual and ReLU, ONE rounding, and an 8-byte NHWC store or four NCHW stores.
// Every output element is ONE accumulator chain in ascending (chunk, tap, ci): no atomics, no split-K.
//
// The helpers carry the units' index and address expressions UNCHANGED, (size_t)(ch * TAPS + tap) * 64 included, and hand results
// back BY VALUE: the same value in another form (a size_t weight offset instead of the int chunk), or a helper that writes through
// int& or an array reference, gives other code, up to 28 registers and a wave per SIMD in bev_conv_kernel<f16, 4, 3, 2>.  That is
// why the layout branch of a load or store, whose two address expressions differ from unit to unit, stays at the call and there is
// no store4.  DESIGN.md ("The dense conv tile") and profiles/EXPERIMENTS.md hold the comparison of every kernel with its
// stand-alone form.
#pragma once

#include "common.h"

#pragma clang fp contract(off)   // here, so that no includer can lose it: the epilogues are fma THEN rounding, nothing fused

namespace bevamd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int CK = 32;                        // channels of one staged chunk = one MFMA k-step per tap
constexpr int PSTR = CK + 8;                  // 16-bit elements per pixel in LDS (80 bytes: the padding spreads the banks)

template <bool BF16>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 acc) {
  if constexpr (BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

template <bool BF16>
__device__ __forceinline__ unsigned short round16(float v) {
  if constexpr (BF16)
    return __builtin_bit_cast(unsigned short, (__bf16)v);
  else
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}

template <bool BF16>
__device__ __forceinline__ float widen16(unsigned short v) {
  if constexpr (BF16)
    return (float)__builtin_bit_cast(__bf16, v);
  else
    return (float)__builtin_bit_cast(_Float16, v);
}

// the NCHW half of a unit: the 8 channels at q, q + cstr, .. (cstr: the map's size) packed into 16 bytes
__device__ __forceinline__ u32x4 gather8(const unsigned short* q, size_t cstr) {
  unsigned int e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = q[(size_t)j * cstr];
  u32x4 v;
  v[0] = e[0] | (e[1] << 16);
  v[1] = e[2] | (e[3] << 16);
  v[2] = e[4] | (e[5] << 16);
  v[3] = e[6] | (e[7] << 16);
  return v;
}

// 8 channels [c, c + 8) of one pixel as a 16-byte unit: `base` is the element offset of channel 0 of that pixel, `cstr` the stride
// between channels (1: NHWC, one load; the map's size: NCHW, eight loads); the caller checked the bounds
__device__ __forceinline__ u32x4 load_unit(const unsigned short* src, int nhwc, size_t base, size_t cstr, int c) {
  if (nhwc) return *reinterpret_cast<const u32x4*>(src + base + c);
  return gather8(src + base + (size_t)c * cstr, cstr);
}

// unit idx of a staged tile of NPIX pixels -> (pixel, channel group): the four units of a pixel are neighbours when the source is
// NHWC (consecutive lanes read consecutive 16 bytes), the NPIX units of a group when it is NCHW (consecutive lanes read along x)
struct Unit {
  int p, grp;
};
template <int NPIX>
__device__ __forceinline__ Unit unit_of(int idx, int nhwc) {
  Unit u;
  if (nhwc) { u.grp = idx & 3; u.p = idx >> 2; } else { u.grp = idx / NPIX; u.p = idx - u.grp * NPIX; }
  return u;
}

// The KS x KS taps of the staged chunk `ch`: acc[m][n] += W[tile m][ch][tap] * X[pixel row n at stride S][tap].  wp: the lane's
// A fragment of (first tile, chunk 0, tap 0); wtile: fragments per tile; xb: the lane's B fragment of (row 0, tap 0) in a tile IW
// pixels wide
template <bool BF16, int MT, int KS, int S, int IW>
__device__ __forceinline__ void chunk_mma(f32x4 (&acc)[MT][4], const u32x4* wp, size_t wtile, int ch, const unsigned short* xb) {
  constexpr int TAPS = KS * KS;
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap) {
    const int ky = tap / KS, kx = tap % KS;
    u32x4 af[MT], bf[4];
#pragma unroll
    for (int m = 0; m < MT; ++m) af[m] = wp[(size_t)m * wtile + (size_t)(ch * TAPS + tap) * 64];
#pragma unroll
    for (int n = 0; n < 4; ++n) bf[n] = *reinterpret_cast<const u32x4*>(xb + ((n * S + ky) * IW + kx) * PSTR);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = mfma16<BF16>(af[m], bf[n], acc[m][n]);
  }
}

// the folded BatchNorm of the four channels co .. co + 3: two float4 loads, made once per channel tile and used for its pixels
struct Affine4 {
  float s[4], t[4];
};
__device__ __forceinline__ Affine4 load_affine4(const float* scale, const float* shift, int co) {
  const float4 sc = *reinterpret_cast<const float4*>(scale + co);
  const float4 sh = *reinterpret_cast<const float4*>(shift + co);
  return Affine4{{sc.x, sc.y, sc.z, sc.w}, {sh.x, sh.y, sh.z, sh.w}};
}

// y = fma(acc, scale[co + q], shift[co + q]).
// OPAQUE: y passes through an empty asm, so that the value a caller rounds IS the fp32 fma.  Without it the compiler may fuse the
// fma and a conversion to fp16 into v_fma_mixlo_f16, which was seen to differ from the two-step form in about one element in 2^13.
// cam_neck_conv_kernel, where that was seen (its ReLU is optional, so nothing need stand between the two), sets the flag.  No other
// kernel contains the fused instruction, and carrying the barrier for everyone changes the code of all of them
// (profiles/EXPERIMENTS.md, "The dense conv tile"): they stay without it.
template <bool OPAQUE = false>
__device__ __forceinline__ float affine(float acc, const Affine4& f, int q) {
  float y = fmaf(acc, f.s[q], f.t[q]);
  if constexpr (OPAQUE) asm("" : "+v"(y));
  return y;
}

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// the 8 bytes of an NHWC load as four channels of one pixel in fp32 (the identity residual)
template <bool BF16>
__device__ __forceinline__ void widen4(u32x2 w, float (&r)[4]) {
  r[0] = widen16<BF16>((unsigned short)(w[0] & 0xffffu));
  r[1] = widen16<BF16>((unsigned short)(w[0] >> 16));
  r[2] = widen16<BF16>((unsigned short)(w[1] & 0xffffu));
  r[3] = widen16<BF16>((unsigned short)(w[1] >> 16));
}

// four rounded channels of one pixel as the 8 bytes of an NHWC store
__device__ __forceinline__ u32x2 pack4(unsigned short r0, unsigned short r1, unsigned short r2, unsigned short r3) {
  u32x2 o;
  o[0] = (unsigned int)r0 | ((unsigned int)r1 << 16);
  o[1] = (unsigned int)r2 | ((unsigned int)r3 << 16);
  return o;
}

// ---- host ----
static inline bool ranges_overlap(const void* p, long long pbytes, const void* q, long long qbytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

}  // namespace bevamd
