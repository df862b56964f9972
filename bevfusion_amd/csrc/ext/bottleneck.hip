// The tail of a ResNet Bottleneck in eval mode, gfx950: conv3 1x1 + folded bn3 + residual + ReLU in ONE launch.
//
// Replaces (mmdet 2.x mmdet/models/backbones/resnet.py, Bottleneck.forward):
//     out = bn3(conv3(h));  out += downsample(x) if downsample is not None else x;  out = relu(out)
//   with downsample = Sequential(Conv2d 1x1 stride 1 or 2, BatchNorm2d): five (identity) or seven launches over the widest maps of
//   the camera backbone, every intermediate written and read once.
//
// Native formulation: the dense conv tile of dense_tile.h without a halo.
//   * The output pixels of the whole batch are ONE flat index p = (b OH + oy) OW + ox.  A workgroup of four waves owns 128
//     consecutive p x 32 * MT output channels (MT = 1, 2 or 4): wave w owns the channel half w & 1 and the 64 pixels 64 (w >> 1) ..,
//     four MFMA column tiles of 16.  A tile may span two samples; a pixel's result depends on nothing but its own column.
//   * Phase 1 (acc3): the 128 pixels of h are staged chunk by chunk.  Phase 2 (accd, downsample mode only): the 128 pixels
//     (b, s oy, s ox) of x are staged into the same buffer and multiplied by the 1 x 1 weight into a SECOND accumulator set.  In
//     both phases the next chunk (the first chunk of x after the last of h) is loaded from memory into registers while the current
//     one is multiplied.  Pixels past the last are zero in LDS.
//   * h, x and dst carry their own layout.  The weights come from bev_pack_weight with one tap.
//   * Epilogue: v = fma(acc3, scale3, shift3); r = x at the lane's own pixel and four channels (identity) or
//     r = fma(accd, scale_d, shift_d); y = max(v + r, 0) rounded once.
// One accumulator chain per product; equal calls give equal bits and a sample's result does not depend on the batch around it.
#include "dense_tile.h"

namespace bevamd {

constexpr int BT_PIX = 128;                   // flat output pixels of one workgroup
constexpr int BT_THREADS = 256;
constexpr int BT_UNITS = BT_PIX * (CK / 8);                  // a unit: 8 channels of one pixel, 16 bytes
constexpr int BT_UPT = BT_UNITS / BT_THREADS;
static_assert(BT_UNITS % BT_THREADS == 0, "every thread stages the same number of units");

struct BtArgs {
  const unsigned short* h;
  const unsigned short* x;
  int h_nhwc, x_nhwc;
  int P, C, Cx;                               // channels of h, of dst and of x
  int OH, OW;                                 // the map of h and dst
  int Hx, Wx, s;                              // the map of x and the downsample's stride
  int nch3, nchd;
  int npix;                                   // batch * OH * OW
  const unsigned short* packed3;
  const float* scale3;
  const float* shift3;
  const unsigned short* packed_d;
  const float* scale_d;
  const float* shift_d;
  unsigned short* dst;
  int dst_nhwc;
};

template <bool BF16, int MT, bool DS>
__global__ __launch_bounds__(BT_THREADS) void bottleneck_tail_kernel(BtArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short xs[BT_PIX * PSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * BT_PIX;
  const int ctile = blockIdx.y;
  const int ohw = a.OH * a.OW;
  const size_t xhw = (size_t)a.Hx * a.Wx;

  // what this thread stages: per unit its LDS pixel, its channel group and the element offset of the pixel's channel 0 in h and x
  int up_h[BT_UPT], ug_h[BT_UPT], up_x[BT_UPT], ug_x[BT_UPT];
  size_t base_h[BT_UPT], base_x[BT_UPT];
  bool live_h[BT_UPT], live_x[BT_UPT];
#pragma unroll
  for (int u = 0; u < BT_UPT; ++u) {
    const int idx = tid + u * BT_THREADS;
    // unit_of<BT_PIX>, written out: through the helper the identity kernels come out with two instructions exchanged
    if (a.h_nhwc) { ug_h[u] = idx & 3; up_h[u] = idx >> 2; } else { ug_h[u] = idx / BT_PIX; up_h[u] = idx - ug_h[u] * BT_PIX; }
    if (a.x_nhwc) { ug_x[u] = idx & 3; up_x[u] = idx >> 2; } else { ug_x[u] = idx / BT_PIX; up_x[u] = idx - ug_x[u] * BT_PIX; }
    {
      const int p = p0 + up_h[u];
      live_h[u] = p < a.npix;
      const int b = live_h[u] ? p / ohw : 0, rem = live_h[u] ? p - b * ohw : 0;
      base_h[u] = a.h_nhwc ? (size_t)(live_h[u] ? p : 0) * a.P : (size_t)b * a.P * ohw + rem;
    }
    {
      const int p = p0 + up_x[u];
      live_x[u] = DS && p < a.npix;
      const int b = live_x[u] ? p / ohw : 0, rem = live_x[u] ? p - b * ohw : 0;
      const int oy = rem / a.OW, ox = rem - oy * a.OW;
      const size_t pix = (size_t)(oy * a.s) * a.Wx + (size_t)(ox * a.s);
      base_x[u] = a.x_nhwc ? ((size_t)b * xhw + pix) * a.Cx : (size_t)b * a.Cx * xhw + pix;
    }
  }

  u32x4 pre[BT_UPT];
  auto load_h = [&](int ch) {
#pragma unroll
    for (int u = 0; u < BT_UPT; ++u) {
      const int c = ch * CK + ug_h[u] * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live_h[u] && c < a.P) v = load_unit(a.h, a.h_nhwc, base_h[u], (size_t)ohw, c);
      pre[u] = v;
    }
  };
  auto store_h = [&]() {
#pragma unroll
    for (int u = 0; u < BT_UPT; ++u) *reinterpret_cast<u32x4*>(xs + up_h[u] * PSTR + ug_h[u] * 8) = pre[u];
  };
  auto load_x = [&](int ch) {
#pragma unroll
    for (int u = 0; u < BT_UPT; ++u) {
      const int c = ch * CK + ug_x[u] * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (live_x[u] && c < a.Cx) v = load_unit(a.x, a.x_nhwc, base_x[u], xhw, c);
      pre[u] = v;
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int u = 0; u < BT_UPT; ++u) *reinterpret_cast<u32x4*>(xs + up_x[u] * PSTR + ug_x[u] * 8) = pre[u];
  };

  const int mh = wave & 1, q0 = (wave >> 1) * 64;        // the wave's channel half and first pixel of the tile
  const int lr = lane & 15, lg = lane >> 4;
  const int mt0 = ctile * (2 * MT) + mh * MT;            // the wave's first tile of 16 channels
  // B fragment: lane holds S[k = 8 lg + j][pixel q0 + 16 n + lr]
  const unsigned short* xb = xs + (q0 + lr) * PSTR + lg * 8;

  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  {
    // A fragment of (channel tile mt, chunk): 64 lanes x 16 bytes
    const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed3) + ((size_t)mt0 * a.nch3) * 64 + lane;
    const size_t wtile = (size_t)a.nch3 * 64;
    load_h(0);
#pragma unroll 1
    for (int ch = 0; ch < a.nch3; ++ch) {
      store_h();
      __syncthreads();
      if (ch + 1 < a.nch3) load_h(ch + 1);
      else if constexpr (DS) load_x(0);
      chunk_mma<BF16, MT, 1, 1, 16>(acc, wp, wtile, ch, xb);
      __syncthreads();   // the next chunk overwrites the tile
    }
  }

  f32x4 accd[DS ? MT : 1][4];
  if constexpr (DS) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) accd[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed_d) + ((size_t)mt0 * a.nchd) * 64 + lane;
    const size_t wtile = (size_t)a.nchd * 64;
#pragma unroll 1
    for (int ch = 0; ch < a.nchd; ++ch) {
      store_x();
      __syncthreads();
      if (ch + 1 < a.nchd) load_x(ch + 1);
      chunk_mma<BF16, MT, 1, 1, 16>(accd, wp, wtile, ch, xb);
      __syncthreads();
    }
  }

  // D fragment: pixel on the lane (lr), channel = 16 tile + 4 lg + reg
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int p = p0 + q0 + n * 16 + lr;
    if (p >= a.npix) continue;
    const int b = p / ohw, rem = p - b * ohw;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int co = (mt0 + m) * 16 + lg * 4;
      const Affine4 bn3 = load_affine4(a.scale3, a.shift3, co);
      float res[4];
      if constexpr (DS) {
        const Affine4 bnd = load_affine4(a.scale_d, a.shift_d, co);
#pragma unroll
        for (int q = 0; q < 4; ++q) res[q] = affine(accd[m][n][q], bnd, q);
      } else {
        // identity: x is [B, C, OH, OW]
        if (a.x_nhwc) {
          widen4<BF16>(*reinterpret_cast<const u32x2*>(a.x + (size_t)p * a.C + co), res);
        } else {
          const unsigned short* r0 = a.x + ((size_t)b * a.C + co) * ohw + rem;
#pragma unroll
          for (int q = 0; q < 4; ++q) res[q] = widen16<BF16>(r0[(size_t)q * ohw]);
        }
      }
      unsigned short r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) r[q] = round16<BF16>(relu(affine(acc[m][n][q], bn3, q) + res[q]));
      if (a.dst_nhwc) {
        *reinterpret_cast<u32x2*>(a.dst + (size_t)p * a.C + co) = pack4(r[0], r[1], r[2], r[3]);
      } else {
        unsigned short* d = a.dst + ((size_t)b * a.C + co) * ohw + rem;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[(size_t)q * ohw] = r[q];
      }
    }
  }
}

template <bool BF16, bool DS>
static void bt_launch(const BtArgs& a, hipStream_t stream) {
  const int tiles = (int)cdiv(a.npix, BT_PIX);
  if (a.C % 128 == 0)
    bottleneck_tail_kernel<BF16, 4, DS><<<dim3(tiles, a.C / 128), dim3(BT_THREADS), 0, stream>>>(a);
  else if (a.C % 64 == 0)
    bottleneck_tail_kernel<BF16, 2, DS><<<dim3(tiles, a.C / 64), dim3(BT_THREADS), 0, stream>>>(a);
  else
    bottleneck_tail_kernel<BF16, 1, DS><<<dim3(tiles, a.C / 32), dim3(BT_THREADS), 0, stream>>>(a);
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_bottleneck_tail_forward(const void* h, int h_layout, int planes, const void* x, int x_layout, int x_channels, int x_height,
                                   int x_width, int dtype, int batch, int channels, int out_height, int out_width, int residual,
                                   int stride, const void* packed3, long long packed3_elems, const float* scale3, const float* shift3,
                                   const void* packed_d, long long packed_d_elems, const float* scale_d, const float* shift_d,
                                   void* dst, int dst_layout, long long dst_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "bottleneck_tail_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(out_height >= 1 && out_width >= 1 && x_height >= 1 && x_width >= 1,
                 "bottleneck_tail_forward: bad sizes (output %d x %d, x %d x %d)", out_height, out_width, x_height, x_width);
  BEVAMD_REQUIRE((h_layout == 0 || h_layout == 1) && (x_layout == 0 || x_layout == 1) && (dst_layout == 0 || dst_layout == 1),
                 "bottleneck_tail_forward: layouts are 0 (NCHW) or 1 (NHWC), got %d, %d and %d", h_layout, x_layout, dst_layout);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "bottleneck_tail_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  if (residual != 0 && residual != 1) {
    set_error("bottleneck_tail_forward: not supported (residual mode %d; 0: identity, 1: downsample)", residual);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (stride != 1 && stride != 2) {
    set_error("bottleneck_tail_forward: not supported (stride %d; 1 or 2)", stride);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (channels < 32 || channels % 32) {
    set_error("bottleneck_tail_forward: not supported (channels %d must be a multiple of 32)", channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (planes < 16 || planes % 16) {
    set_error("bottleneck_tail_forward: not supported (planes %d must be a multiple of 16)", planes);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (x_channels < 16 || x_channels % 16) {
    set_error("bottleneck_tail_forward: not supported (x_channels %d must be a multiple of 16)", x_channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  const bool ds = residual == 1;
  if (ds) {
    BEVAMD_REQUIRE((x_height - 1) / stride + 1 == out_height && (x_width - 1) / stride + 1 == out_width,
                   "bottleneck_tail_forward: a %d x %d map of x at stride %d does not give the %d x %d output", x_height, x_width,
                   stride, out_height, out_width);
  } else {
    BEVAMD_REQUIRE(stride == 1 && x_channels == channels && x_height == out_height && x_width == out_width,
                   "bottleneck_tail_forward: the identity residual needs x [%d, %d, %d] equal to the output [%d, %d, %d] at stride 1, got stride %d",
                   x_channels, x_height, x_width, channels, out_height, out_width, stride);
  }
  const int nch3 = (planes + CK - 1) / CK, nchd = ds ? (x_channels + CK - 1) / CK : 0;
  const long long want3 = (long long)channels * nch3 * CK;
  BEVAMD_REQUIRE(packed3_elems == want3, "bottleneck_tail_forward: packed3 holds %lld elements, this block needs %lld", packed3_elems, want3);
  const long long wantd = (long long)channels * nchd * CK;
  BEVAMD_REQUIRE(packed_d_elems == wantd, "bottleneck_tail_forward: packed_d holds %lld elements, this block needs %lld", packed_d_elems, wantd);
  const long long npix = (long long)batch * out_height * (long long)out_width;
  const long long want_dst = npix * channels;
  BEVAMD_REQUIRE(dst_elems == want_dst, "bottleneck_tail_forward: dst holds %lld elements, [%d, %d, %d, %d] needs %lld", dst_elems, batch,
                 channels, out_height, out_width, want_dst);
  BEVAMD_REQUIRE(npix <= 0x7fffffffLL - BT_PIX && (long long)x_height * x_width <= 0x7fffffffLL,
                 "bottleneck_tail_forward: %d maps of %d x %d have too many pixels", batch, out_height, out_width);
  BEVAMD_REQUIRE(packed3 != nullptr && ((uintptr_t)packed3 & 15) == 0, "bottleneck_tail_forward: packed3 is null or not 16-byte aligned");
  BEVAMD_REQUIRE(scale3 != nullptr && shift3 != nullptr && (((uintptr_t)scale3 | (uintptr_t)shift3) & 15) == 0,
                 "bottleneck_tail_forward: scale3 or shift3 is null or not 16-byte aligned");
  if (ds) {
    BEVAMD_REQUIRE(packed_d != nullptr && ((uintptr_t)packed_d & 15) == 0, "bottleneck_tail_forward: packed_d is null or not 16-byte aligned");
    BEVAMD_REQUIRE(scale_d != nullptr && shift_d != nullptr && (((uintptr_t)scale_d | (uintptr_t)shift_d) & 15) == 0,
                   "bottleneck_tail_forward: scale_d or shift_d is null or not 16-byte aligned");
  }
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(h != nullptr && x != nullptr && dst != nullptr, "bottleneck_tail_forward: h, x or dst is null");
  BEVAMD_REQUIRE(h_layout == 0 || ((uintptr_t)h & 15) == 0, "bottleneck_tail_forward: an NHWC h is not 16-byte aligned");
  BEVAMD_REQUIRE(x_layout == 0 || ((uintptr_t)x & 15) == 0, "bottleneck_tail_forward: an NHWC x is not 16-byte aligned");
  BEVAMD_REQUIRE((((uintptr_t)h | (uintptr_t)x | (uintptr_t)dst) & 1) == 0, "bottleneck_tail_forward: h, x or dst is not 2-byte aligned");
  BEVAMD_REQUIRE(dst_layout == 0 || ((uintptr_t)dst & 7) == 0, "bottleneck_tail_forward: an NHWC dst is not 8-byte aligned");
  const long long h_bytes = 2LL * npix * planes;
  const long long x_bytes = 2LL * batch * x_channels * x_height * (long long)x_width;
  BEVAMD_REQUIRE(!ranges_overlap(dst, 2 * want_dst, h, h_bytes) && !ranges_overlap(dst, 2 * want_dst, x, x_bytes),
                 "bottleneck_tail_forward: dst overlaps h or x");

  BtArgs a;
  a.h = (const unsigned short*)h;
  a.x = (const unsigned short*)x;
  a.h_nhwc = h_layout;
  a.x_nhwc = x_layout;
  a.P = planes;
  a.C = channels;
  a.Cx = x_channels;
  a.OH = out_height;
  a.OW = out_width;
  a.Hx = x_height;
  a.Wx = x_width;
  a.s = stride;
  a.nch3 = nch3;
  a.nchd = nchd;
  a.npix = (int)npix;
  a.packed3 = (const unsigned short*)packed3;
  a.scale3 = scale3;
  a.shift3 = shift3;
  a.packed_d = (const unsigned short*)packed_d;
  a.scale_d = scale_d;
  a.shift_d = shift_d;
  a.dst = (unsigned short*)dst;
  a.dst_nhwc = dst_layout;
  if (dtype == 1) {
    if (ds) bt_launch<true, true>(a, stream);
    else bt_launch<true, false>(a, stream);
  } else {
    if (ds) bt_launch<false, true>(a, stream);
    else bt_launch<false, false>(a, stream);
  }
  BEVAMD_LAUNCH_CHECK("bottleneck_tail");
  return BEVAMD_OK;
}

}  // extern "C"
