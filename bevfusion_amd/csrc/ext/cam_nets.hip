// The learned nets of the camera -> BEV view transform in eval mode, gfx950: the depth stem and the depthnet's softmax head.
//
// Replaces (reference):
//   mmdet3d/models/vtransforms/depth_lss.py:43-53, 84  dtransform: Conv2d(1, 8, 1) + BN + ReLU, Conv2d(8, 32, 5, stride 4, padding 2)
//                                                      + BN + ReLU, Conv2d(32, 64, 5, stride 2, padding 2) + BN + ReLU
//   mmdet3d/models/vtransforms/depth_lss.py:88-97      the end of depthnet: Conv2d(Cin, D + C, 1), softmax over D, the split
//   mmdet3d/models/vtransforms/lss.py:63-75            the same end of LSSTransform's one-layer depthnet
//
// Native formulation: implicit GEMMs D[channel][pixel] with the operand layouts of dense_tile.h.
//   * stem, launch 1 (layers 1 + 2): a workgroup of four waves owns 8 x 16 layer-2 pixels x 32 channels.  The 33 x 65 depth tile is
//     read once; layer 1 is a per-pixel function of the scalar depth, a1[c] = max(fma(d, s1[c], t1[c]), 0), computed in fp32 while
//     staging, rounded once and kept in LDS as [pixel][8 channels] (16 bytes); a cell outside the image holds ZERO (layer 2 pads
//     the output of layer 1, not the depth).  K = 25 taps x 8 channels = 200, padded to 224: k-step c of lane group g is tap 4 c + g,
//     so a lane's B fragment is one 16-byte LDS read; the taps 25 .. 27 are zero on both operands.
//   * stem, launch 2 (layer 3): 8 x 16 output pixels x 64 channels per workgroup from the 19 x 35 x 32 haloed tile of the layer-2
//     map, staged as ONE chunk of the dense conv tile; K = 25 taps x 32 channels, one k-step per tap.
//   * both epilogues: y = max(fma(acc, scale[co], shift[co]), 0) in fp32, rounded once, 8-byte NHWC stores of 4 channels.
//   * head: a wave owns 32 pixels (two MFMA column tiles) and ALL D + C rows (up to 16 tiles of 16: 128 accumulator registers).
//     The B fragments come straight from the NHWC input (every element is read once), the A fragments stream from L2; no LDS, no
//     barrier.  Logits z = acc + bias stay in registers.  A pixel's rows live in the four lanes lr, lr + 16, lr + 32, lr + 48: the
//     maximum and the sum over the rows < D are reduced over the lane's own registers in ascending row order and then over the lane
//     groups by two xor shuffles; rows >= D (the context rows of the straddling tile, the padding past D + C) never enter either.
//     depth = exp(z - max) / sum with ocml's expf and an IEEE division.
// Every output element is ONE accumulator chain in a fixed order: no atomics, no split-K; equal calls give equal bits and a
// sample's result does not depend on the batch around it.  No address outside the tensors is formed.
#include "dense_tile.h"

namespace bevamd {

constexpr int CN_TH = 8, CN_TW = 16;                 // output pixels of one workgroup (both stem launches)
constexpr int CN_THREADS = 256;
constexpr int CN_K5 = 5, CN_TAPS = 25;
// launch 1: the layer-1 tile of an 8 x 16 layer-2 tile at stride 4
constexpr int CN_S2_IH = (CN_TH - 1) * 4 + CN_K5, CN_S2_IW = (CN_TW - 1) * 4 + CN_K5;      // 33 x 65
constexpr int CN_S2_STEPS = 7;                       // ceil(200 / 32)
// launch 2: the layer-2 tile of an 8 x 16 layer-3 tile at stride 2
constexpr int CN_S3_IH = (CN_TH - 1) * 2 + CN_K5, CN_S3_IW = (CN_TW - 1) * 2 + CN_K5;      // 19 x 35
constexpr int CN_HEAD_NT = 2;                        // MFMA column tiles (16 pixels) of one wave of the head
constexpr int CN_HEAD_PIX = 16 * CN_HEAD_NT;

// y = round16(max(fma(acc, scale, shift), 0)) of the four channels co .. co + 3 of one pixel, one 8-byte store
template <bool BF16>
__device__ __forceinline__ void cn_store4(unsigned short* dst, f32x4 acc, const float* scale, const float* shift, int co) {
  const Affine4 bn = load_affine4(scale, shift, co);
  unsigned int r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) r[q] = round16<BF16>(relu(affine(acc[q], bn, q)));
  *reinterpret_cast<u32x2*>(dst + co) = pack4(r[0], r[1], r[2], r[3]);
}

struct CnStemArgs {
  const float* depth;                                 // [n, H, W]
  int H, W, OH2, OW2, OH3, OW3;
  const float* s1;                                    // [8] each
  const float* t1;
  const unsigned short* packed2;                      // [2 tiles][7 steps][64 lanes][8]
  const float* s2;                                    // [32] each
  const float* t2;
  const unsigned short* packed3;                      // [4 tiles][1 chunk][25 taps][64 lanes][8]
  const float* s3;                                    // [64] each
  const float* t3;
  unsigned short* mid;                                // [n, OH2, OW2, 32]
  unsigned short* out;                                // [n, OH3, OW3, 64]
  int tiles_x;
};

// layers 1 + 2: depth [n, H, W] fp32 -> mid [n, OH2, OW2, 32]
template <bool BF16>
__global__ __launch_bounds__(CN_THREADS) void cam_stem12_kernel(CnStemArgs a) {
  constexpr int NPIX = CN_S2_IH * CN_S2_IW;
  __shared__ __attribute__((aligned(16))) unsigned short xs[NPIX * 8];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int b = blockIdx.z;
  const int oy0 = ty * CN_TH, ox0 = tx * CN_TW;
  const int iy0 = oy0 * 4 - 2, ix0 = ox0 * 4 - 2;

  float s1[8], t1[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    s1[c] = a.s1[c];
    t1[c] = a.t1[c];
  }
  const float* img = a.depth + (size_t)b * a.H * a.W;
  for (int p = tid; p < NPIX; p += CN_THREADS) {
    const int iy = p / CN_S2_IW, ix = p - iy * CN_S2_IW;
    const int gy = iy0 + iy, gx = ix0 + ix;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const float d = img[(size_t)gy * a.W + gx];
      unsigned int r[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float y = fmaf(d, s1[c], t1[c]);
        r[c] = round16<BF16>(y > 0.f ? y : 0.f);
      }
      v[0] = r[0] | (r[1] << 16);
      v[1] = r[2] | (r[3] << 16);
      v[2] = r[4] | (r[5] << 16);
      v[3] = r[6] | (r[7] << 16);
    }
    *reinterpret_cast<u32x4*>(xs + p * 8) = v;
  }
  __syncthreads();

  const int lr = lane & 15, lg = lane >> 4;
  const int r0 = wave * 2;                                    // the wave's two pixel rows
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed2) + lane;
  f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int c = 0; c < CN_S2_STEPS; ++c) {
    const int tap = 4 * c + lg;                                // k = 32 c + 8 lg + j = 8 tap + j
    const bool live = tap < CN_TAPS;
    const int tp = live ? tap : CN_TAPS - 1;
    const int ky = tp / CN_K5, kx = tp - ky * CN_K5;
    u32x4 af[2], bf[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) af[m] = wp[(m * CN_S2_STEPS + c) * 64];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(xs + (((r0 + n) * 4 + ky) * CN_S2_IW + lr * 4 + kx) * 8);
      bf[n] = live ? v : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = mfma16<BF16>(af[m], bf[n], acc[m][n]);
  }

  const int ox = ox0 + lr;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int oy = oy0 + r0 + n;
    if (oy >= a.OH2 || ox >= a.OW2) continue;
    unsigned short* dst = a.mid + (((size_t)b * a.OH2 + oy) * a.OW2 + ox) * 32;
#pragma unroll
    for (int m = 0; m < 2; ++m) cn_store4<BF16>(dst, acc[m][n], a.s2, a.t2, m * 16 + lg * 4);
  }
}

// layer 3: mid [n, OH2, OW2, 32] -> out [n, OH3, OW3, 64]
template <bool BF16>
__global__ __launch_bounds__(CN_THREADS) void cam_stem3_kernel(CnStemArgs a) {
  constexpr int NPIX = CN_S3_IH * CN_S3_IW, UNITS = NPIX * 4;                    // a unit: 8 channels of one pixel, 16 bytes
  __shared__ __attribute__((aligned(16))) unsigned short xs[NPIX * PSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int b = blockIdx.z;
  const int oy0 = ty * CN_TH, ox0 = tx * CN_TW;
  const int iy0 = oy0 * 2 - 2, ix0 = ox0 * 2 - 2;

  for (int idx = tid; idx < UNITS; idx += CN_THREADS) {
    const int grp = idx & 3, p = idx >> 2;
    const int iy = p / CN_S3_IW, ix = p - iy * CN_S3_IW;
    const int gy = iy0 + iy, gx = ix0 + ix;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (gy >= 0 && gy < a.OH2 && gx >= 0 && gx < a.OW2)
      v = *reinterpret_cast<const u32x4*>(a.mid + (((size_t)b * a.OH2 + gy) * a.OW2 + gx) * 32 + grp * 8);
    *reinterpret_cast<u32x4*>(xs + p * PSTR + grp * 8) = v;
  }
  __syncthreads();

  const int lr = lane & 15, lg = lane >> 4;
  const int mh = wave & 1, r0 = (wave >> 1) * 4;              // channel half (two tiles of 16) and the four pixel rows
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed3) + (size_t)(mh * 2) * (CN_TAPS * 64) + lane;
  const unsigned short* xb = xs + ((r0 * 2) * CN_S3_IW + lr * 2) * PSTR + lg * 8;
  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  chunk_mma<BF16, 2, CN_K5, 2, CN_S3_IW>(acc, wp, (size_t)CN_TAPS * 64, 0, xb);   // one chunk: the layer-2 map has 32 channels

  const int ox = ox0 + lr;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int oy = oy0 + r0 + n;
    if (oy >= a.OH3 || ox >= a.OW3) continue;
    unsigned short* dst = a.out + (((size_t)b * a.OH3 + oy) * a.OW3 + ox) * 64;
#pragma unroll
    for (int m = 0; m < 2; ++m) cn_store4<BF16>(dst, acc[m][n], a.s3, a.t3, (mh * 2 + m) * 16 + lg * 4);
  }
}

struct CnHeadArgs {
  const unsigned short* x;                            // [pixels, cin]
  long long pixels, hw;                               // pixels = n * hw
  int cin, nch, D, C, mt;                             // mt = ceil((D + C) / 16) tiles of 16 rows
  const unsigned short* packed;                       // [mt][nch][64 lanes][8]
  const float* bias;                                  // [D + C]
  float* depth;                                       // [n, D, hw]
  float* ctx;                                         // [pixels, C]
};

// MT: the tiles of 16 rows the kernel is built for (the tiles >= a.mt are skipped by a wave-uniform branch)
template <bool BF16, int MT>
__global__ __launch_bounds__(64) void cam_head_kernel(CnHeadArgs a) {
  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const long long p0 = (long long)blockIdx.x * CN_HEAD_PIX;
  long long pix[CN_HEAD_NT];
  bool in[CN_HEAD_NT];
#pragma unroll
  for (int n = 0; n < CN_HEAD_NT; ++n) {
    pix[n] = p0 + n * 16 + lr;
    in[n] = pix[n] < a.pixels;
  }
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed) + lane;

  f32x4 acc[MT][CN_HEAD_NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < CN_HEAD_NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int ch = 0; ch < a.nch; ++ch) {
    u32x4 bf[CN_HEAD_NT];
#pragma unroll
    for (int n = 0; n < CN_HEAD_NT; ++n) {
      bf[n] = u32x4{0u, 0u, 0u, 0u};
      if (in[n]) bf[n] = *reinterpret_cast<const u32x4*>(a.x + (size_t)pix[n] * a.cin + ch * 32 + lg * 8);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m < a.mt) {
        const u32x4 af = wp[((size_t)m * a.nch + ch) * 64];
#pragma unroll
        for (int n = 0; n < CN_HEAD_NT; ++n) acc[m][n] = mfma16<BF16>(af, bf[n], acc[m][n]);
      }
    }
  }

  // logits: row = 16 m + 4 lg + q of pixel lr
  const int rows = a.D + a.C;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (m < a.mt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m * 16 + lg * 4 + q;
        const float bv = row < rows ? a.bias[row] : 0.f;
#pragma unroll
        for (int n = 0; n < CN_HEAD_NT; ++n) acc[m][n][q] = acc[m][n][q] + bv;
      }
    }
  }

#pragma unroll
  for (int n = 0; n < CN_HEAD_NT; ++n) {
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m < a.mt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m * 16 + lg * 4 + q;
          if (row < a.D) mx = fmaxf(mx, acc[m][n][q]);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));      // D >= 1: row 0 is a depth row, the maximum is a logit
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m < a.mt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m * 16 + lg * 4 + q;
          if (row < a.D) {
            const float e = expf(acc[m][n][q] - mx);
            acc[m][n][q] = e;
            sum = sum + e;
          }
        }
      }
    }
    sum = sum + __shfl_xor(sum, 16, 64);
    sum = sum + __shfl_xor(sum, 32, 64);
    if (!in[n]) continue;
    const long long img = pix[n] / a.hw, cell = pix[n] - img * a.hw;
    float* dp = a.depth + (size_t)img * a.D * a.hw + cell;
    float* cp = a.ctx + (size_t)pix[n] * a.C;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m < a.mt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m * 16 + lg * 4 + q;
          if (row < a.D)
            dp[(size_t)row * a.hw] = acc[m][n][q] / sum;
          else if (row < rows)
            cp[row - a.D] = acc[m][n][q];
        }
      }
    }
  }
}

template <bool BF16>
static void cn_head_launch(const CnHeadArgs& a, hipStream_t stream) {
  const int blocks = (int)((a.pixels + CN_HEAD_PIX - 1) / CN_HEAD_PIX);
  if (a.mt <= 4)
    cam_head_kernel<BF16, 4><<<dim3(blocks), dim3(64), 0, stream>>>(a);
  else if (a.mt <= 8)
    cam_head_kernel<BF16, 8><<<dim3(blocks), dim3(64), 0, stream>>>(a);
  else
    cam_head_kernel<BF16, 16><<<dim3(blocks), dim3(64), 0, stream>>>(a);
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_cam_depth_stem_forward(const float* depth, long long depth_elems, int batch, int height, int width, int dtype,
                                  const float* scale1, const float* shift1, const void* packed2, long long packed2_elems,
                                  const float* scale2, const float* shift2, const void* packed3, long long packed3_elems,
                                  const float* scale3, const float* shift3, void* scratch, long long scratch_elems, void* out,
                                  long long out_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "cam_depth_stem_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(height >= 1 && width >= 1, "cam_depth_stem_forward: bad sizes (H %d, W %d)", height, width);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "cam_depth_stem_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  const int OH2 = (height - 1) / 4 + 1, OW2 = (width - 1) / 4 + 1;
  const int OH3 = (OH2 - 1) / 2 + 1, OW3 = (OW2 - 1) / 2 + 1;
  const long long want_depth = (long long)batch * height * width;
  const long long want_mid = (long long)batch * OH2 * OW2 * 32, want_out = (long long)batch * OH3 * OW3 * 64;
  BEVAMD_REQUIRE(depth_elems == want_depth, "cam_depth_stem_forward: depth holds %lld elements, [%d, %d, %d] needs %lld", depth_elems,
                 batch, height, width, want_depth);
  BEVAMD_REQUIRE(packed2_elems == 32LL * CN_S2_STEPS * 32 && packed3_elems == 64LL * CN_TAPS * 32,
                 "cam_depth_stem_forward: packed weights hold %lld and %lld elements, the stem needs %d and %d", packed2_elems,
                 packed3_elems, 32 * CN_S2_STEPS * 32, 64 * CN_TAPS * 32);
  BEVAMD_REQUIRE(scratch_elems == want_mid, "cam_depth_stem_forward: scratch holds %lld elements, [%d, %d, %d, 32] needs %lld",
                 scratch_elems, batch, OH2, OW2, want_mid);
  BEVAMD_REQUIRE(out_elems == want_out, "cam_depth_stem_forward: out holds %lld elements, [%d, %d, %d, 64] needs %lld", out_elems,
                 batch, OH3, OW3, want_out);
  const long long tiles2_x = cdiv(OW2, CN_TW), tiles2 = tiles2_x * cdiv(OH2, CN_TH);
  BEVAMD_REQUIRE(tiles2 <= 0x7fffffffLL, "cam_depth_stem_forward: a %d x %d map has too many tiles", height, width);
  BEVAMD_REQUIRE(packed2 != nullptr && packed3 != nullptr && (((uintptr_t)packed2 | (uintptr_t)packed3) & 15) == 0,
                 "cam_depth_stem_forward: packed weights are null or not 16-byte aligned");
  BEVAMD_REQUIRE(scale1 != nullptr && shift1 != nullptr && scale2 != nullptr && shift2 != nullptr && scale3 != nullptr &&
                     shift3 != nullptr && (((uintptr_t)scale2 | (uintptr_t)shift2 | (uintptr_t)scale3 | (uintptr_t)shift3) & 15) == 0,
                 "cam_depth_stem_forward: a scale or shift is null or not 16-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(depth != nullptr && scratch != nullptr && out != nullptr, "cam_depth_stem_forward: depth, scratch or out is null");
  BEVAMD_REQUIRE((((uintptr_t)scratch | (uintptr_t)out) & 15) == 0 && ((uintptr_t)depth & 3) == 0,
                 "cam_depth_stem_forward: scratch or out is not 16-byte aligned, or depth not 4-byte aligned");

  CnStemArgs a;
  a.depth = depth;
  a.H = height;
  a.W = width;
  a.OH2 = OH2;
  a.OW2 = OW2;
  a.OH3 = OH3;
  a.OW3 = OW3;
  a.s1 = scale1;
  a.t1 = shift1;
  a.packed2 = (const unsigned short*)packed2;
  a.s2 = scale2;
  a.t2 = shift2;
  a.packed3 = (const unsigned short*)packed3;
  a.s3 = scale3;
  a.t3 = shift3;
  a.mid = (unsigned short*)scratch;
  a.out = (unsigned short*)out;
  a.tiles_x = (int)tiles2_x;
  if (dtype == 1)
    cam_stem12_kernel<true><<<dim3((unsigned)tiles2, 1, batch), dim3(CN_THREADS), 0, stream>>>(a);
  else
    cam_stem12_kernel<false><<<dim3((unsigned)tiles2, 1, batch), dim3(CN_THREADS), 0, stream>>>(a);
  BEVAMD_LAUNCH_CHECK("cam_stem12");
  a.tiles_x = cdiv(OW3, CN_TW);
  const unsigned tiles3 = (unsigned)a.tiles_x * (unsigned)cdiv(OH3, CN_TH);
  if (dtype == 1)
    cam_stem3_kernel<true><<<dim3(tiles3, 1, batch), dim3(CN_THREADS), 0, stream>>>(a);
  else
    cam_stem3_kernel<false><<<dim3(tiles3, 1, batch), dim3(CN_THREADS), 0, stream>>>(a);
  BEVAMD_LAUNCH_CHECK("cam_stem3");
  return BEVAMD_OK;
}

int bevamd_cam_depth_head_forward(const void* x, long long x_elems, int batch, int height, int width, int in_channels, int depth_bins,
                                  int context_channels, int dtype, const void* packed, long long packed_elems, const float* bias,
                                  float* depth, long long depth_elems, float* context, long long context_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "cam_depth_head_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(height >= 1 && width >= 1, "cam_depth_head_forward: bad sizes (H %d, W %d)", height, width);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "cam_depth_head_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  if (in_channels < 32 || in_channels > 512 || in_channels % 32 || depth_bins < 1 || depth_bins > 128 || context_channels < 4 ||
      context_channels > 128 || context_channels % 4) {
    set_error("cam_depth_head_forward: not supported (in_channels %d: a multiple of 32 up to 512; depth_bins %d: 1 .. 128; "
              "context_channels %d: a multiple of 4 up to 128)", in_channels, depth_bins, context_channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  const int rows = depth_bins + context_channels, mt = (rows + 15) / 16, nch = in_channels / 32;
  const long long hw = (long long)height * width, pixels = hw * batch;
  BEVAMD_REQUIRE(pixels / CN_HEAD_PIX < 0x7fffffffLL, "cam_depth_head_forward: %lld pixels are too many", pixels);
  BEVAMD_REQUIRE(x_elems == pixels * in_channels, "cam_depth_head_forward: x holds %lld elements, [%d, %d, %d, %d] needs %lld", x_elems,
                 batch, height, width, in_channels, pixels * in_channels);
  BEVAMD_REQUIRE(packed_elems == (long long)mt * 16 * in_channels,
                 "cam_depth_head_forward: packed holds %lld elements, %d rows padded to %d x %d channels need %lld", packed_elems, rows,
                 mt * 16, in_channels, (long long)mt * 16 * in_channels);
  BEVAMD_REQUIRE(depth_elems == pixels * depth_bins, "cam_depth_head_forward: depth holds %lld elements, [%d, %d, %d, %d] needs %lld",
                 depth_elems, batch, depth_bins, height, width, pixels * depth_bins);
  BEVAMD_REQUIRE(context_elems == pixels * context_channels,
                 "cam_depth_head_forward: context holds %lld elements, [%d, %d, %d, %d] needs %lld", context_elems, batch, height, width,
                 context_channels, pixels * context_channels);
  BEVAMD_REQUIRE(packed != nullptr && ((uintptr_t)packed & 15) == 0, "cam_depth_head_forward: packed is null or not 16-byte aligned");
  BEVAMD_REQUIRE(bias != nullptr && ((uintptr_t)bias & 3) == 0, "cam_depth_head_forward: bias is null or not 4-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(x != nullptr && depth != nullptr && context != nullptr, "cam_depth_head_forward: x, depth or context is null");
  BEVAMD_REQUIRE(((uintptr_t)x & 15) == 0 && (((uintptr_t)depth | (uintptr_t)context) & 3) == 0,
                 "cam_depth_head_forward: x is not 16-byte aligned, or depth or context not 4-byte aligned");

  CnHeadArgs a;
  a.x = (const unsigned short*)x;
  a.pixels = pixels;
  a.hw = hw;
  a.cin = in_channels;
  a.nch = nch;
  a.D = depth_bins;
  a.C = context_channels;
  a.mt = mt;
  a.packed = (const unsigned short*)packed;
  a.bias = bias;
  a.depth = depth;
  a.ctx = context;
  if (dtype == 1)
    cn_head_launch<true>(a, stream);
  else
    cn_head_launch<false>(a, stream);
  BEVAMD_LAUNCH_CHECK("cam_head");
  return BEVAMD_OK;
}

}  // extern "C"
