// One layer of the dense BEV trunk in eval mode, gfx950: convolution, folded BatchNorm and ReLU in ONE launch.
//
// Replaces (reference):
//   mmdet3d/models/fusers/conv.py:22-23      ConvFuser.forward: torch.cat + Conv2d 3x3 + BatchNorm2d + ReLU
//   mmdet3d/models/backbones/second.py:93-97 SECOND.forward: per layer Conv2d 3x3 (stride 1 or 2) + BatchNorm2d + ReLU
//   mmdet3d/models/necks/second.py:93-98     SECONDFPN.forward: per level Conv2d / ConvTranspose2d + BatchNorm2d + ReLU, torch.cat
//
// Native formulation: the dense conv tile of dense_tile.h.
//   * A workgroup of four waves owns 8 x 16 output pixels x 32 * MT output channels (MT = 1, 2 or 4): wave w owns the channel half
//     w & 1 (MT tiles of 16 channels) and the four pixel rows 4 (w >> 1) ..; every pixel row of 16 is one MFMA column tile.
//   * The haloed input tile ((8 - 1) s + k) x ((16 - 1) s + k) pixels is staged chunk by chunk.  The next chunk is loaded from
//     memory into registers while the current one is multiplied (one LDS buffer, two barriers per chunk).
//   * Up to two sources are read as one channel-concatenated input (every staged group of 8 channels lies in one source), each
//     NCHW or NHWC.
//   * Epilogue: y = max(fma(acc, scale[co], shift[co]), 0), written into the channel window [dst_off, dst_off + cout) of an NHWC
//     or NCHW destination.
//   * A deconvolution with kernel = stride = 2 is four 1 x 1 products (blockIdx.y carries the tap) written to (2y + dy, 2x + dx).
// Equal calls give equal bits and a sample's result does not depend on the batch around it.
#include "dense_tile.h"

namespace bevamd {

constexpr int BC_TH = 8, BC_TW = 16;          // output pixels of one workgroup
constexpr int BC_THREADS = 256;

struct BcArgs {
  const unsigned short* src0;
  const unsigned short* src1;
  int c0, c1, src_nhwc;
  int H, W;                                   // the sources' map
  int OH, OW;                                 // the convolution's output (before the deconvolution's factor `up`)
  int cout, nch, tiles_x, up;
  const unsigned short* packed;
  const float* scale;
  const float* shift;
  unsigned short* dst;
  int dst_c, dst_off, dst_nhwc;
};

template <bool BF16, int MT, int KS, int S>
__global__ __launch_bounds__(BC_THREADS) void bev_conv_kernel(BcArgs a) {
  constexpr int P = KS / 2, TAPS = KS * KS;
  constexpr int IH = (BC_TH - 1) * S + KS, IW = (BC_TW - 1) * S + KS;   // the haloed input tile
  constexpr int NPIX = IH * IW, UNITS = NPIX * (CK / 8);             // a unit: 8 channels of one pixel, 16 bytes
  constexpr int UPT = (UNITS + BC_THREADS - 1) / BC_THREADS;
  __shared__ __attribute__((aligned(16))) unsigned short xs[NPIX * PSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int cout_tiles = a.cout / (32 * MT);
  const int g = blockIdx.y / cout_tiles, ctile = blockIdx.y - g * cout_tiles;
  const int b = blockIdx.z;
  const int oy0 = ty * BC_TH, ox0 = tx * BC_TW;
  const int iy0 = oy0 * S - P, ix0 = ox0 * S - P;
  const int ctot = a.c0 + a.c1;
  const size_t hw = (size_t)a.H * a.W;

  u32x4 pre[UPT];
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int idx = tid + u * BC_THREADS;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (idx < UNITS) {
        const Unit un = unit_of<NPIX>(idx, a.src_nhwc);
        const int iy = un.p / IW, ix = un.p - iy * IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const int c = ch * CK + un.grp * 8;
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && c < ctot) {
          const bool first = c < a.c0;
          const unsigned short* src = first ? a.src0 : a.src1;
          const int cc = first ? c : c - a.c0, cs = first ? a.c0 : a.c1;
          if (a.src_nhwc) v = *reinterpret_cast<const u32x4*>(src + (((size_t)b * a.H + gy) * a.W + gx) * cs + cc);
          else v = gather8(src + ((size_t)b * cs + cc) * hw + (size_t)gy * a.W + gx, hw);
        }
      }
      pre[u] = v;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int idx = tid + u * BC_THREADS;
      if (idx < UNITS) {
        const Unit un = unit_of<NPIX>(idx, a.src_nhwc);
        *reinterpret_cast<u32x4*>(xs + un.p * PSTR + un.grp * 8) = pre[u];
      }
    }
  };

  const int mh = wave & 1, r0 = (wave >> 1) * 4;
  const int lr = lane & 15, lg = lane >> 4;
  const int mt0 = ctile * (2 * MT) + mh * MT;            // the wave's first tile of 16 channels
  // A fragment of (group g, channel tile mt, chunk, tap): 64 lanes x 16 bytes
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed) + ((size_t)(g * (a.cout / 16) + mt0) * a.nch) * (TAPS * 64) + lane;
  const size_t wtile = (size_t)a.nch * (TAPS * 64);
  // B fragment: lane holds X[k = 8 lg + j][pixel lr] of pixel row r0 + n
  const unsigned short* xb = xs + ((r0 * S) * IW + lr * S) * PSTR + lg * 8;

  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_chunk(0);
#pragma unroll 1
  for (int ch = 0; ch < a.nch; ++ch) {
    store_chunk();
    __syncthreads();
    if (ch + 1 < a.nch) load_chunk(ch + 1);
    chunk_mma<BF16, MT, KS, S, IW>(acc, wp, wtile, ch, xb);
    __syncthreads();   // the next chunk overwrites the tile
  }

  const int dy = a.up == 2 ? g >> 1 : 0, dx = a.up == 2 ? g & 1 : 0;
  const int OHt = a.OH * a.up, OWt = a.OW * a.up;
  const int ox = ox0 + lr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = (mt0 + m) * 16 + lg * 4;
    const Affine4 bn = load_affine4(a.scale, a.shift, co);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int oy = oy0 + r0 + n;
      if (oy >= a.OH || ox >= a.OW) continue;
      const int Y = oy * a.up + dy, X = ox * a.up + dx;
      unsigned short r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) r[q] = round16<BF16>(relu(affine(acc[m][n][q], bn, q)));
      if (a.dst_nhwc) {
        *reinterpret_cast<u32x2*>(a.dst + (((size_t)b * OHt + Y) * OWt + X) * a.dst_c + a.dst_off + co) = pack4(r[0], r[1], r[2], r[3]);
      } else {
        unsigned short* d = a.dst + (((size_t)b * a.dst_c + a.dst_off + co) * OHt + Y) * OWt + X;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[(size_t)q * OHt * OWt] = r[q];
      }
    }
  }
}

template <bool BF16, int KS, int S>
static void bc_launch(const BcArgs& a, int groups, int batch, hipStream_t stream) {
  const int tiles = a.tiles_x * (int)cdiv(a.OH, BC_TH);
#ifdef BEVAMD_BC_S2_TILE256   // the 256-channel tile of profiles/EXPERIMENTS.md: the stride-2 input tile staged once, not twice
  if constexpr (S == 2) {
    if (a.cout % 256 == 0) {
      bev_conv_kernel<BF16, 8, KS, S><<<dim3(tiles, a.cout / 256 * groups, batch), dim3(BC_THREADS), 0, stream>>>(a);
      return;
    }
  }
#endif
  if (a.cout % 128 == 0)
    bev_conv_kernel<BF16, 4, KS, S><<<dim3(tiles, a.cout / 128 * groups, batch), dim3(BC_THREADS), 0, stream>>>(a);
  else if (a.cout % 64 == 0)
    bev_conv_kernel<BF16, 2, KS, S><<<dim3(tiles, a.cout / 64 * groups, batch), dim3(BC_THREADS), 0, stream>>>(a);
  else
    bev_conv_kernel<BF16, 1, KS, S><<<dim3(tiles, a.cout / 32 * groups, batch), dim3(BC_THREADS), 0, stream>>>(a);
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_bev_conv_forward(const void* src0, int channels0, const void* src1, int channels1, int src_layout, int dtype, int batch,
                            int height, int width, int out_channels, int kernel, int stride, int mode, const void* packed,
                            long long packed_elems, const float* scale, const float* shift, void* dst, int dst_channels_total,
                            int dst_channel_offset, int dst_layout, long long dst_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "bev_conv_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(height >= 1 && width >= 1, "bev_conv_forward: bad sizes (H %d, W %d)", height, width);
  BEVAMD_REQUIRE((src_layout == 0 || src_layout == 1) && (dst_layout == 0 || dst_layout == 1),
                 "bev_conv_forward: layouts are 0 (NCHW) or 1 (NHWC), got %d and %d", src_layout, dst_layout);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "bev_conv_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  const bool conv3 = mode == 0 && kernel == 3 && (stride == 1 || stride == 2);
  const bool conv1 = mode == 0 && kernel == 1 && stride == 1;
  const bool deconv = mode == 1 && kernel == 2 && stride == 2;
  if (!(conv3 || conv1 || deconv)) {
    set_error("bev_conv_forward: not supported (mode %d, kernel %d, stride %d; conv 3x3 stride 1 or 2, conv 1x1 stride 1, deconv 2x2 stride 2)",
              mode, kernel, stride);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (channels0 < 16 || channels0 % 16 || channels1 < 0 || channels1 % 16 || out_channels < 32 || out_channels % 32) {
    set_error("bev_conv_forward: not supported (source channels %d and %d must be multiples of 16, out_channels %d a multiple of 32)",
              channels0, channels1, out_channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (dst_layout == 1 && (dst_channels_total % 4 || dst_channel_offset % 4)) {
    set_error("bev_conv_forward: not supported (an NHWC destination needs dst_channels_total %d and dst_channel_offset %d in multiples of 4)",
              dst_channels_total, dst_channel_offset);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(dst_channel_offset >= 0 && (long long)dst_channel_offset + out_channels <= dst_channels_total,
                 "bev_conv_forward: the window [%d, %d + %d) does not fit %d destination channels", dst_channel_offset, dst_channel_offset,
                 out_channels, dst_channels_total);
  const int up = deconv ? 2 : 1, groups = up * up, taps = deconv ? 1 : kernel * kernel;
  const int OH = deconv ? height : (height + 2 * (kernel / 2) - kernel) / stride + 1;
  const int OW = deconv ? width : (width + 2 * (kernel / 2) - kernel) / stride + 1;
  const int nch = (channels0 + channels1 + CK - 1) / CK;
  const long long want_packed = (long long)groups * out_channels * nch * taps * CK;
  BEVAMD_REQUIRE(packed_elems == want_packed, "bev_conv_forward: packed holds %lld elements, this layer needs %lld", packed_elems, want_packed);
  const long long want_dst = (long long)batch * dst_channels_total * (OH * up) * (long long)(OW * up);
  BEVAMD_REQUIRE(dst_elems == want_dst, "bev_conv_forward: dst holds %lld elements, [%d, %d, %d, %d] needs %lld", dst_elems, batch,
                 dst_channels_total, OH * up, OW * up, want_dst);
  const long long tiles_x = cdiv(OW, BC_TW), tiles = tiles_x * cdiv(OH, BC_TH);
  BEVAMD_REQUIRE(tiles <= 0x7fffffffLL, "bev_conv_forward: a %d x %d map has too many tiles", height, width);
  BEVAMD_REQUIRE(packed != nullptr && ((uintptr_t)packed & 15) == 0, "bev_conv_forward: packed is null or not 16-byte aligned");
  BEVAMD_REQUIRE(scale != nullptr && shift != nullptr && (((uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
                 "bev_conv_forward: scale or shift is null or not 16-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(src0 != nullptr && dst != nullptr && (channels1 == 0 || src1 != nullptr), "bev_conv_forward: a source or dst is null");
  BEVAMD_REQUIRE(src_layout == 0 || ((((uintptr_t)src0 | (uintptr_t)src1) & 15) == 0), "bev_conv_forward: an NHWC source is not 16-byte aligned");
  BEVAMD_REQUIRE(dst_layout == 0 || ((uintptr_t)dst & 7) == 0, "bev_conv_forward: an NHWC dst is not 8-byte aligned");

  BcArgs a;
  a.src0 = (const unsigned short*)src0;
  a.src1 = (const unsigned short*)src1;
  a.c0 = channels0;
  a.c1 = channels1;
  a.src_nhwc = src_layout;
  a.H = height;
  a.W = width;
  a.OH = OH;
  a.OW = OW;
  a.cout = out_channels;
  a.nch = nch;
  a.tiles_x = (int)tiles_x;
  a.up = up;
  a.packed = (const unsigned short*)packed;
  a.scale = scale;
  a.shift = shift;
  a.dst = (unsigned short*)dst;
  a.dst_c = dst_channels_total;
  a.dst_off = dst_channel_offset;
  a.dst_nhwc = dst_layout;
  if (dtype == 1) {
    if (kernel == 3 && stride == 1) bc_launch<true, 3, 1>(a, groups, batch, stream);
    else if (kernel == 3) bc_launch<true, 3, 2>(a, groups, batch, stream);
    else bc_launch<true, 1, 1>(a, groups, batch, stream);
  } else {
    if (kernel == 3 && stride == 1) bc_launch<false, 3, 1>(a, groups, batch, stream);
    else if (kernel == 3) bc_launch<false, 3, 2>(a, groups, batch, stream);
    else bc_launch<false, 1, 1>(a, groups, batch, stream);
  }
  BEVAMD_LAUNCH_CHECK("bev_conv");
  return BEVAMD_OK;
}

}  // extern "C"
