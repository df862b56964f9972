// The second half of a ResNet BasicBlock in eval mode, gfx950: conv2 3x3 + folded bn2 + residual + ReLU in ONE launch.
//
// Replaces (reference):
//   mmdet3d/models/backbones/resnet.py:35-40  GeneralizedResNet.forward, per mmcv BasicBlock the tail
//     out = bn2(conv2(h));  out += downsample(x) if downsample is not None else x;  out = relu(out)
//   with downsample = Sequential(Conv2d 1x1 stride 1 or 2, BatchNorm2d): five (identity) or seven launches and every
//   intermediate map written and read once.
//
// Native formulation: the dense conv tile of dense_tile.h.
//   * A workgroup of four waves owns 8 x 16 output pixels x 32 * MT output channels (MT = 1, 2 or 4): wave w owns the channel half
//     w & 1 and the four pixel rows 4 (w >> 1) ..; every pixel row of 16 is one MFMA column tile.
//   * Phase 1 (acc2): the haloed 10 x 18 tile of h is staged chunk by chunk; the nine taps read the same chunk from shifted
//     addresses.  Phase 2 (accd, downsample mode only): only the 8 x 16 pixels (s oy, s ox) of x are staged, into the same LDS
//     buffer, and multiplied by the 1 x 1 weight into a SECOND accumulator set.  In both phases the next chunk (the first chunk of
//     x after the last of h) is loaded from memory into registers while the current one is multiplied.
//   * h and x carry their own layout.  The weights come from bev_pack_weight (a 1 x 1 weight packs with taps = 1).
//   * Epilogue: v = fma(acc2, scale2, shift2); r = x at the lane's own pixel and four channels (identity) or
//     r = fma(accd, scale_d, shift_d); y = max(v + r, 0) rounded once.
// One accumulator chain per product; equal calls give equal bits and a sample's result does not depend on the batch around it.
#include "dense_tile.h"

namespace bevamd {

constexpr int RB_TH = 8, RB_TW = 16;          // output pixels of one workgroup
constexpr int RB_THREADS = 256;
constexpr int RB_IH = RB_TH + 2, RB_IW = RB_TW + 2;          // the haloed tile of h
constexpr int RB_NPIX = RB_IH * RB_IW;
constexpr int RB_UNITS = RB_NPIX * (CK / 8);                 // a unit: 8 channels of one pixel, 16 bytes
constexpr int RB_UPT = (RB_UNITS + RB_THREADS - 1) / RB_THREADS;
constexpr int RB_XPIX = RB_TH * RB_TW;                       // the pixels of x a downsample stages
constexpr int RB_XUNITS = RB_XPIX * (CK / 8);
constexpr int RB_XUPT = RB_XUNITS / RB_THREADS;
static_assert(RB_XUNITS % RB_THREADS == 0 && RB_XUPT <= RB_UPT, "the x tile fits the prefetch registers of the h tile");

struct RbArgs {
  const unsigned short* h;
  const unsigned short* x;
  int h_nhwc, x_nhwc;
  int C, Cx;                                  // channels of h / dst and of x
  int OH, OW;                                 // the map of h and dst
  int Hx, Wx, s;                              // the map of x and the downsample's stride
  int nch2, nchd, tiles_x;
  const unsigned short* packed2;
  const float* scale2;
  const float* shift2;
  const unsigned short* packed_d;
  const float* scale_d;
  const float* shift_d;
  unsigned short* dst;
  int dst_nhwc;
};

// 8 channels [c, c + 8) of pixel (gy, gx) of sample b of a [B, cs, H, W] tensor as one unit; the caller checked the bounds.  Its
// own address arithmetic, not load_unit's base + c * cstr: that adds 35 to 48 instructions to every kernel (profiles/EXPERIMENTS.md)
__device__ __forceinline__ u32x4 rb_load_unit(const unsigned short* src, int nhwc, int b, int cs, int H, int W, int c, int gy, int gx) {
  if (nhwc) return *reinterpret_cast<const u32x4*>(src + (((size_t)b * H + gy) * W + gx) * cs + c);
  const size_t hw = (size_t)H * W;
  return gather8(src + ((size_t)b * cs + c) * hw + (size_t)gy * W + gx, hw);
}

template <bool BF16, int MT, bool DS>
__global__ __launch_bounds__(RB_THREADS) void res_block_kernel(RbArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short xs[RB_NPIX * PSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int ctile = blockIdx.y;
  const int b = blockIdx.z;
  const int oy0 = ty * RB_TH, ox0 = tx * RB_TW;

  u32x4 pre[RB_UPT];
  auto load_h = [&](int ch) {
#pragma unroll
    for (int u = 0; u < RB_UPT; ++u) {
      const int idx = tid + u * RB_THREADS;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (idx < RB_UNITS) {
        const Unit un = unit_of<RB_NPIX>(idx, a.h_nhwc);
        const int iy = un.p / RB_IW, ix = un.p - iy * RB_IW;
        const int gy = oy0 - 1 + iy, gx = ox0 - 1 + ix;
        const int c = ch * CK + un.grp * 8;
        if (gy >= 0 && gy < a.OH && gx >= 0 && gx < a.OW && c < a.C) v = rb_load_unit(a.h, a.h_nhwc, b, a.C, a.OH, a.OW, c, gy, gx);
      }
      pre[u] = v;
    }
  };
  auto store_h = [&]() {
#pragma unroll
    for (int u = 0; u < RB_UPT; ++u) {
      const int idx = tid + u * RB_THREADS;
      if (idx < RB_UNITS) {
        const Unit un = unit_of<RB_NPIX>(idx, a.h_nhwc);
        *reinterpret_cast<u32x4*>(xs + un.p * PSTR + un.grp * 8) = pre[u];
      }
    }
  };
  // downsample: the 8 x 16 pixels (s oy, s ox) of x, pixel p = 16 py + px at xs[p]
  auto load_x = [&](int ch) {
#pragma unroll
    for (int u = 0; u < RB_XUPT; ++u) {
      const int idx = tid + u * RB_THREADS;
      const Unit un = unit_of<RB_XPIX>(idx, a.x_nhwc);
      const int oy = oy0 + (un.p >> 4), ox = ox0 + (un.p & 15);
      const int c = ch * CK + un.grp * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (oy < a.OH && ox < a.OW && c < a.Cx) v = rb_load_unit(a.x, a.x_nhwc, b, a.Cx, a.Hx, a.Wx, c, oy * a.s, ox * a.s);
      pre[u] = v;
    }
  };
  auto store_x = [&]() {
#pragma unroll
    for (int u = 0; u < RB_XUPT; ++u) {
      const int idx = tid + u * RB_THREADS;
      const Unit un = unit_of<RB_XPIX>(idx, a.x_nhwc);
      *reinterpret_cast<u32x4*>(xs + un.p * PSTR + un.grp * 8) = pre[u];
    }
  };

  const int mh = wave & 1, r0 = (wave >> 1) * 4;
  const int lr = lane & 15, lg = lane >> 4;
  const int mt0 = ctile * (2 * MT) + mh * MT;            // the wave's first tile of 16 channels

  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  {
    // A fragment of (channel tile mt, chunk, tap): 64 lanes x 16 bytes
    const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed2) + ((size_t)mt0 * a.nch2) * (9 * 64) + lane;
    const size_t wtile = (size_t)a.nch2 * (9 * 64);
    // B fragment: lane holds H[k = 8 lg + j][pixel lr] of pixel row r0 + n
    const unsigned short* xb = xs + (r0 * RB_IW + lr) * PSTR + lg * 8;
    load_h(0);
#pragma unroll 1
    for (int ch = 0; ch < a.nch2; ++ch) {
      store_h();
      __syncthreads();
      if (ch + 1 < a.nch2) load_h(ch + 1);
      else if constexpr (DS) load_x(0);
      chunk_mma<BF16, MT, 3, 1, RB_IW>(acc, wp, wtile, ch, xb);
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
    const unsigned short* xb = xs + (r0 * RB_TW + lr) * PSTR + lg * 8;
#pragma unroll 1
    for (int ch = 0; ch < a.nchd; ++ch) {
      store_x();
      __syncthreads();
      if (ch + 1 < a.nchd) load_x(ch + 1);
      chunk_mma<BF16, MT, 1, 1, RB_TW>(accd, wp, wtile, ch, xb);
      __syncthreads();
    }
  }

  // D fragment: pixel on the lane (lr), channel = 16 tile + 4 lg + reg
  const int ox = ox0 + lr;
  const size_t ohw = (size_t)a.OH * a.OW;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = (mt0 + m) * 16 + lg * 4;
    const Affine4 bn2 = load_affine4(a.scale2, a.shift2, co);
    Affine4 bnd = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if constexpr (DS) bnd = load_affine4(a.scale_d, a.shift_d, co);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int oy = oy0 + r0 + n;
      if (oy >= a.OH || ox >= a.OW) continue;
      float res[4];
      if constexpr (DS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) res[q] = affine(accd[m][n][q], bnd, q);
      } else {
        // identity: x is [B, C, OH, OW]
        if (a.x_nhwc) {
          widen4<BF16>(*reinterpret_cast<const u32x2*>(a.x + (((size_t)b * a.OH + oy) * a.OW + ox) * a.C + co), res);
        } else {
          const unsigned short* q0 = a.x + ((size_t)b * a.C + co) * ohw + (size_t)oy * a.OW + ox;
#pragma unroll
          for (int q = 0; q < 4; ++q) res[q] = widen16<BF16>(q0[(size_t)q * ohw]);
        }
      }
      unsigned short r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) r[q] = round16<BF16>(relu(affine(acc[m][n][q], bn2, q) + res[q]));
      if (a.dst_nhwc) {
        *reinterpret_cast<u32x2*>(a.dst + (((size_t)b * a.OH + oy) * a.OW + ox) * a.C + co) = pack4(r[0], r[1], r[2], r[3]);
      } else {
        unsigned short* d = a.dst + ((size_t)b * a.C + co) * ohw + (size_t)oy * a.OW + ox;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[(size_t)q * ohw] = r[q];
      }
    }
  }
}

template <bool BF16, bool DS>
static void rb_launch(const RbArgs& a, int batch, hipStream_t stream) {
  const int tiles = a.tiles_x * (int)cdiv(a.OH, RB_TH);
  if (a.C % 128 == 0)
    res_block_kernel<BF16, 4, DS><<<dim3(tiles, a.C / 128, batch), dim3(RB_THREADS), 0, stream>>>(a);
  else if (a.C % 64 == 0)
    res_block_kernel<BF16, 2, DS><<<dim3(tiles, a.C / 64, batch), dim3(RB_THREADS), 0, stream>>>(a);
  else
    res_block_kernel<BF16, 1, DS><<<dim3(tiles, a.C / 32, batch), dim3(RB_THREADS), 0, stream>>>(a);
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_res_block_forward(const void* h, int h_layout, const void* x, int x_layout, int x_channels, int x_height, int x_width,
                             int dtype, int batch, int channels, int out_height, int out_width, int residual, int stride,
                             const void* packed2, long long packed2_elems, const float* scale2, const float* shift2,
                             const void* packed_d, long long packed_d_elems, const float* scale_d, const float* shift_d, void* dst,
                             int dst_layout, long long dst_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "res_block_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(out_height >= 1 && out_width >= 1 && x_height >= 1 && x_width >= 1,
                 "res_block_forward: bad sizes (output %d x %d, x %d x %d)", out_height, out_width, x_height, x_width);
  BEVAMD_REQUIRE((h_layout == 0 || h_layout == 1) && (x_layout == 0 || x_layout == 1) && (dst_layout == 0 || dst_layout == 1),
                 "res_block_forward: layouts are 0 (NCHW) or 1 (NHWC), got %d, %d and %d", h_layout, x_layout, dst_layout);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "res_block_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  if (residual != 0 && residual != 1) {
    set_error("res_block_forward: not supported (residual mode %d; 0: identity, 1: downsample)", residual);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (stride != 1 && stride != 2) {
    set_error("res_block_forward: not supported (stride %d; 1 or 2)", stride);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (channels < 32 || channels % 32) {
    set_error("res_block_forward: not supported (channels %d must be a multiple of 32)", channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (x_channels < 16 || x_channels % 16) {
    set_error("res_block_forward: not supported (x_channels %d must be a multiple of 16)", x_channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  const bool ds = residual == 1;
  if (ds) {
    BEVAMD_REQUIRE((x_height - 1) / stride + 1 == out_height && (x_width - 1) / stride + 1 == out_width,
                   "res_block_forward: a %d x %d map of x at stride %d does not give the %d x %d output", x_height, x_width, stride,
                   out_height, out_width);
  } else {
    BEVAMD_REQUIRE(stride == 1 && x_channels == channels && x_height == out_height && x_width == out_width,
                   "res_block_forward: the identity residual needs x [%d, %d, %d] equal to the output [%d, %d, %d] at stride 1, got stride %d",
                   x_channels, x_height, x_width, channels, out_height, out_width, stride);
  }
  const int nch2 = channels / CK, nchd = ds ? (x_channels + CK - 1) / CK : 0;
  const long long want2 = (long long)channels * nch2 * 9 * CK;
  BEVAMD_REQUIRE(packed2_elems == want2, "res_block_forward: packed2 holds %lld elements, this block needs %lld", packed2_elems, want2);
  const long long wantd = (long long)channels * nchd * CK;
  BEVAMD_REQUIRE(packed_d_elems == wantd, "res_block_forward: packed_d holds %lld elements, this block needs %lld", packed_d_elems, wantd);
  const long long want_dst = (long long)batch * channels * out_height * (long long)out_width;
  BEVAMD_REQUIRE(dst_elems == want_dst, "res_block_forward: dst holds %lld elements, [%d, %d, %d, %d] needs %lld", dst_elems, batch,
                 channels, out_height, out_width, want_dst);
  const long long tiles_x = cdiv(out_width, RB_TW), tiles = tiles_x * cdiv(out_height, RB_TH);
  BEVAMD_REQUIRE(tiles <= 0x7fffffffLL, "res_block_forward: a %d x %d map has too many tiles", out_height, out_width);
  BEVAMD_REQUIRE(packed2 != nullptr && ((uintptr_t)packed2 & 15) == 0, "res_block_forward: packed2 is null or not 16-byte aligned");
  BEVAMD_REQUIRE(scale2 != nullptr && shift2 != nullptr && (((uintptr_t)scale2 | (uintptr_t)shift2) & 15) == 0,
                 "res_block_forward: scale2 or shift2 is null or not 16-byte aligned");
  if (ds) {
    BEVAMD_REQUIRE(packed_d != nullptr && ((uintptr_t)packed_d & 15) == 0, "res_block_forward: packed_d is null or not 16-byte aligned");
    BEVAMD_REQUIRE(scale_d != nullptr && shift_d != nullptr && (((uintptr_t)scale_d | (uintptr_t)shift_d) & 15) == 0,
                   "res_block_forward: scale_d or shift_d is null or not 16-byte aligned");
  }
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(h != nullptr && x != nullptr && dst != nullptr, "res_block_forward: h, x or dst is null");
  BEVAMD_REQUIRE(h_layout == 0 || ((uintptr_t)h & 15) == 0, "res_block_forward: an NHWC h is not 16-byte aligned");
  BEVAMD_REQUIRE(x_layout == 0 || ((uintptr_t)x & 15) == 0, "res_block_forward: an NHWC x is not 16-byte aligned");
  BEVAMD_REQUIRE((((uintptr_t)h | (uintptr_t)x | (uintptr_t)dst) & 1) == 0, "res_block_forward: h, x or dst is not 2-byte aligned");
  BEVAMD_REQUIRE(dst_layout == 0 || ((uintptr_t)dst & 7) == 0, "res_block_forward: an NHWC dst is not 8-byte aligned");
  const long long x_bytes = 2LL * batch * x_channels * x_height * (long long)x_width;
  BEVAMD_REQUIRE(!ranges_overlap(dst, 2 * want_dst, h, 2 * want_dst) && !ranges_overlap(dst, 2 * want_dst, x, x_bytes),
                 "res_block_forward: dst overlaps h or x");

  RbArgs a;
  a.h = (const unsigned short*)h;
  a.x = (const unsigned short*)x;
  a.h_nhwc = h_layout;
  a.x_nhwc = x_layout;
  a.C = channels;
  a.Cx = x_channels;
  a.OH = out_height;
  a.OW = out_width;
  a.Hx = x_height;
  a.Wx = x_width;
  a.s = stride;
  a.nch2 = nch2;
  a.nchd = nchd;
  a.tiles_x = (int)tiles_x;
  a.packed2 = (const unsigned short*)packed2;
  a.scale2 = scale2;
  a.shift2 = shift2;
  a.packed_d = (const unsigned short*)packed_d;
  a.scale_d = scale_d;
  a.shift_d = shift_d;
  a.dst = (unsigned short*)dst;
  a.dst_nhwc = dst_layout;
  if (dtype == 1) {
    if (ds) rb_launch<true, true>(a, batch, stream);
    else rb_launch<true, false>(a, batch, stream);
  } else {
    if (ds) rb_launch<false, true>(a, batch, stream);
    else rb_launch<false, false>(a, batch, stream);
  }
  BEVAMD_LAUNCH_CHECK("res_block");
  return BEVAMD_OK;
}

}  // extern "C"
