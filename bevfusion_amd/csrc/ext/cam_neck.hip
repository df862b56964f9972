// One layer of the camera necks in eval mode, gfx950: bilinear resampling (align_corners), channel concatenation, convolution,
// folded BatchNorm and ReLU in ONE launch.
//
// Replaces (reference):
//   mmdet3d/models/necks/generalized_lss.py:91-98  GeneralizedLSSFPN.forward: F.interpolate + torch.cat + ConvModule 1x1
//   mmdet3d/models/necks/lss.py:54-64              LSSFPN.forward: F.interpolate + torch.cat + Conv2d 1x1 + BatchNorm2d + ReLU;
//                                                  nn.Upsample + Conv2d 3x3 + BatchNorm2d + ReLU
//
// Native formulation: the dense conv tile of dense_tile.h at stride 1, kernel 1 or 3: four waves own 8 x 16 output pixels x
// 32 * MT output channels, the next chunk is loaded into registers while the current one is multiplied, and the epilogue is
// y = fma(acc, scale, shift) (ReLU optional) rounded once into a channel window of dst.
// What is new is the staging: each of the two sources has its OWN map and layout.  A source whose map equals the output map is
// copied (no arithmetic).  Any other source is resampled while its unit (8 channels of one staged pixel) is built: the four
// neighbours are loaded (four 16-byte loads from an NHWC source, 4 x 8 two-byte loads from an NCHW one), kept in registers while the
// current chunk is multiplied, combined lane-locally in fp32 without FMA contraction
//     v = hy * (hx * a[y0][x0] + lx * a[y0][x1]) + ly * (hx * a[y1][x0] + lx * a[y1][x1])
// rounded ONCE to the storage type and written as one 16-byte LDS store.  y0, y1, ly of the tile's rows and x0, x1, lx of its
// columns do not depend on the chunk: they are computed once per workgroup into small LDS tables.  The zero padding of a 3 x 3
// layer applies to the RESAMPLED map.  y1 = y0 + (y0 < h - 1) and x1 alike: no address outside a source is formed.
// Equal calls give equal bits and a sample's result does not depend on the batch around it (MT is chosen from the grid size, and
// the bits do not depend on MT).
#include "dense_tile.h"

namespace bevamd {

constexpr int NK_TH = 8, NK_TW = 16;          // output pixels of one workgroup
constexpr int NK_THREADS = 256;
constexpr int NK_FILL = 256;                  // workgroups wanted before a wider channel tile is taken (compute units of the chip)

struct NkArgs {
  const unsigned short* src0;
  const unsigned short* src1;
  int c0, c1;
  int h0, w0, h1, w1;                         // the sources' maps (an absent source: 1 x 1)
  int nhwc0, nhwc1;
  int rs0, rs1;                               // the source is resampled (its map differs from the output map)
  float ry0, rx0, ry1, rx1;                   // (h - 1) / (OH - 1) and (w - 1) / (OW - 1) in fp32, 0 where the output extent is 1
  int OH, OW;
  int cout, nch, tiles_x, relu;
  const unsigned short* packed;
  const float* scale;
  const float* shift;
  unsigned short* dst;
  int dst_c, dst_off, dst_nhwc;
};

// 8 channels [cc, cc + 8) of the pixel at offset `off` (= y * w + x) of sample b: one 16-byte load (NHWC) or eight 2-byte loads.
// Its own address arithmetic, not load_unit's base + c * cstr: that form adds up to 173 instructions a kernel (profiles/EXPERIMENTS.md)
__device__ __forceinline__ u32x4 nk_load8(const unsigned short* src, int nhwc, int b, int cs, int cc, size_t hw, int off) {
  if (nhwc) return *reinterpret_cast<const u32x4*>(src + ((size_t)b * hw + off) * cs + cc);
  return gather8(src + ((size_t)b * cs + cc) * hw + off, hw);
}

// RS: at least one source is resampled (four neighbours per unit are held in registers); without it the staging is a copy
template <bool BF16, int MT, int KS, bool RS>
__global__ __launch_bounds__(NK_THREADS) void cam_neck_conv_kernel(NkArgs a) {
  constexpr int P = KS / 2, TAPS = KS * KS;
  constexpr int IH = NK_TH - 1 + KS, IW = NK_TW - 1 + KS;               // the haloed input tile
  constexpr int NPIX = IH * IW, UNITS = NPIX * (CK / 8);             // a unit: 8 channels of one pixel, 16 bytes
  constexpr int UPT = (UNITS + NK_THREADS - 1) / NK_THREADS;
  constexpr int NB = RS ? 4 : 1;                                        // 16-byte registers per unit
  __shared__ __attribute__((aligned(16))) unsigned short xs[NPIX * PSTR];
  __shared__ int t_y0[2][IH], t_y1[2][IH], t_x0[2][IW], t_x1[2][IW];    // per source: row offsets y * w, columns x
  __shared__ float t_ly[2][IH], t_lx[2][IW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int ctile = blockIdx.y;
  const int b = blockIdx.z;
  const int oy0 = ty * NK_TH, ox0 = tx * NK_TW;
  const int iy0 = oy0 - P, ix0 = ox0 - P;
  const int ctot = a.c0 + a.c1;
  const size_t hw0 = (size_t)a.h0 * a.w0, hw1 = (size_t)a.h1 * a.w1;

  if constexpr (RS) {
    if (tid < 2 * (IH + IW)) {
      const int s = tid / (IH + IW), k = tid - s * (IH + IW);
      const bool row = k < IH;
      const int i = row ? k : k - IH;
      const int n = s ? (row ? a.h1 : a.w1) : (row ? a.h0 : a.w0);      // the source's extent along this axis
      const int N = row ? a.OH : a.OW;
      const float r = s ? (row ? a.ry1 : a.rx1) : (row ? a.ry0 : a.rx0);
      int G = (row ? iy0 : ix0) + i;
      G = G < 0 ? 0 : (G > N - 1 ? N - 1 : G);                          // the halo outside the map is never read: any valid entry
      const float sf = r * (float)G;
      int i0 = (int)sf;
      i0 = i0 < n - 1 ? i0 : n - 1;
      const int i1 = i0 + (i0 < n - 1 ? 1 : 0);
      const float l = sf - (float)i0;
      if (row) {
        const int w = s ? a.w1 : a.w0;
        t_y0[s][i] = i0 * w;
        t_y1[s][i] = i1 * w;
        t_ly[s][i] = l;
      } else {
        t_x0[s][i] = i0;
        t_x1[s][i] = i1;
        t_lx[s][i] = l;
      }
    }
    __syncthreads();
  }

  u32x4 pre[UPT][NB];
  // the unit -> (pixel, channel group) map of a chunk follows the layout of the source its first channel lies in (unit_of written
  // out: through the helper the selects of the 1 x 1 kernels come out in another order)
  auto unit = [&](int ch, int idx, int& p, int& grp) {
    const int nh = ch * CK < a.c0 ? a.nhwc0 : a.nhwc1;
    if (nh) { grp = idx & 3; p = idx >> 2; } else { grp = idx / NPIX; p = idx - grp * NPIX; }
  };
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int idx = tid + u * NK_THREADS;
#pragma unroll
      for (int q = 0; q < NB; ++q) pre[u][q] = u32x4{0u, 0u, 0u, 0u};
      if (idx < UNITS) {
        int p, grp;
        unit(ch, idx, p, grp);
        const int iy = p / IW, ix = p - iy * IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const int c = ch * CK + grp * 8;
        if (gy >= 0 && gy < a.OH && gx >= 0 && gx < a.OW && c < ctot) {
          const bool first = c < a.c0;
          const unsigned short* src = first ? a.src0 : a.src1;
          const int cc = first ? c : c - a.c0, cs = first ? a.c0 : a.c1;
          const int nh = first ? a.nhwc0 : a.nhwc1, sw = first ? a.w0 : a.w1;
          const size_t hw = first ? hw0 : hw1;
          const bool rs = RS && (first ? a.rs0 : a.rs1);
          int y0 = gy * sw, y1 = 0, x0 = gx, x1 = 0;                                // the source's map is the output map
          if constexpr (RS) {
            if (rs) {
              const int s = first ? 0 : 1;
              y0 = t_y0[s][iy], y1 = t_y1[s][iy], x0 = t_x0[s][ix], x1 = t_x1[s][ix];
            }
          }
          pre[u][0] = nk_load8(src, nh, b, cs, cc, hw, y0 + x0);
          if constexpr (RS) {
            if (rs) {
              pre[u][1] = nk_load8(src, nh, b, cs, cc, hw, y0 + x1);
              pre[u][2] = nk_load8(src, nh, b, cs, cc, hw, y1 + x0);
              pre[u][3] = nk_load8(src, nh, b, cs, cc, hw, y1 + x1);
            }
          }
        }
      }
    }
  };
  auto store_chunk = [&](int ch) {
#pragma unroll
    for (int u = 0; u < UPT; ++u) {
      const int idx = tid + u * NK_THREADS;
      if (idx < UNITS) {
        int p, grp;
        unit(ch, idx, p, grp);
        u32x4 v = pre[u][0];
        if constexpr (RS) {
          const int c = ch * CK + grp * 8;
          const bool first = c < a.c0;
          if (first ? a.rs0 : a.rs1) {                   // a unit that was not loaded is four zeros and stays zero
            const int iy = p / IW, ix = p - iy * IW, s = first ? 0 : 1;
            const float ly = t_ly[s][iy], lx = t_lx[s][ix];
            const float hy = 1.f - ly, hx = 1.f - lx;
            unsigned int r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int wd = j >> 1, sh = (j & 1) * 16;
              const float a00 = widen16<BF16>((unsigned short)(pre[u][0][wd] >> sh)), a01 = widen16<BF16>((unsigned short)(pre[u][1][wd] >> sh));
              const float a10 = widen16<BF16>((unsigned short)(pre[u][2][wd] >> sh)), a11 = widen16<BF16>((unsigned short)(pre[u][3][wd] >> sh));
              const float top = hx * a00 + lx * a01, bot = hx * a10 + lx * a11;
              r[j] = round16<BF16>(hy * top + ly * bot);
            }
            v[0] = r[0] | (r[1] << 16);
            v[1] = r[2] | (r[3] << 16);
            v[2] = r[4] | (r[5] << 16);
            v[3] = r[6] | (r[7] << 16);
          }
        }
        *reinterpret_cast<u32x4*>(xs + p * PSTR + grp * 8) = v;
      }
    }
  };

  const int mh = wave & 1, r0 = (wave >> 1) * 4;
  const int lr = lane & 15, lg = lane >> 4;
  const int mt0 = ctile * (2 * MT) + mh * MT;            // the wave's first tile of 16 channels
  // A fragment of (channel tile mt, chunk, tap): 64 lanes x 16 bytes
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed) + ((size_t)mt0 * a.nch) * (TAPS * 64) + lane;
  const size_t wtile = (size_t)a.nch * (TAPS * 64);
  // B fragment: lane holds X[k = 8 lg + j][pixel lr] of pixel row r0 + n
  const unsigned short* xb = xs + (r0 * IW + lr) * PSTR + lg * 8;

  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_chunk(0);
#pragma unroll 1
  for (int ch = 0; ch < a.nch; ++ch) {
    store_chunk(ch);
    __syncthreads();
    if (ch + 1 < a.nch) load_chunk(ch + 1);
    chunk_mma<BF16, MT, KS, 1, IW>(acc, wp, wtile, ch, xb);
    __syncthreads();   // the next chunk overwrites the tile
  }

  // D fragment: pixel on the lane (lr), channel = 16 tile + 4 lg + reg
  const int ox = ox0 + lr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = (mt0 + m) * 16 + lg * 4;
    const Affine4 bn = load_affine4(a.scale, a.shift, co);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int oy = oy0 + r0 + n;
      if (oy >= a.OH || ox >= a.OW) continue;
      unsigned short r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = affine<true>(acc[m][n][q], bn, q);
        r[q] = round16<BF16>(a.relu ? relu(v) : v);
      }
      if (a.dst_nhwc) {
        *reinterpret_cast<u32x2*>(a.dst + (((size_t)b * a.OH + oy) * a.OW + ox) * a.dst_c + a.dst_off + co) = pack4(r[0], r[1], r[2], r[3]);
      } else {
        unsigned short* d = a.dst + (((size_t)b * a.dst_c + a.dst_off + co) * a.OH + oy) * a.OW + ox;
#pragma unroll
        for (int q = 0; q < 4; ++q) d[(size_t)q * a.OH * a.OW] = r[q];
      }
    }
  }
}

// The channel tile: the widest of 128 / 64 / 32 that divides cout and still gives NK_FILL workgroups, else the narrowest that
// divides it (the most workgroups).  The result's bits do not depend on the choice.
template <bool BF16, int KS, bool RS>
static void nk_launch(const NkArgs& a, int batch, hipStream_t stream) {
  const long long tiles = (long long)a.tiles_x * cdiv(a.OH, NK_TH);
  const long long wgs = tiles * batch;
  if (a.cout % 128 == 0 && wgs * (a.cout / 128) >= NK_FILL)
    cam_neck_conv_kernel<BF16, 4, KS, RS><<<dim3((unsigned)tiles, a.cout / 128, batch), dim3(NK_THREADS), 0, stream>>>(a);
  else if (a.cout % 64 == 0 && wgs * (a.cout / 64) >= NK_FILL)
    cam_neck_conv_kernel<BF16, 2, KS, RS><<<dim3((unsigned)tiles, a.cout / 64, batch), dim3(NK_THREADS), 0, stream>>>(a);
  else
    cam_neck_conv_kernel<BF16, 1, KS, RS><<<dim3((unsigned)tiles, a.cout / 32, batch), dim3(NK_THREADS), 0, stream>>>(a);
}

template <bool BF16>
static void nk_dispatch(const NkArgs& a, int kernel, int batch, hipStream_t stream) {
  const bool rs = a.rs0 || a.rs1;
  if (kernel == 3) {
    if (rs) nk_launch<BF16, 3, true>(a, batch, stream);
    else nk_launch<BF16, 3, false>(a, batch, stream);
  } else {
    if (rs) nk_launch<BF16, 1, true>(a, batch, stream);
    else nk_launch<BF16, 1, false>(a, batch, stream);
  }
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_neck_conv_forward(const void* src0, int channels0, int height0, int width0, int layout0, const void* src1, int channels1,
                             int height1, int width1, int layout1, int dtype, int batch, int out_height, int out_width,
                             int out_channels, int kernel, const void* packed, long long packed_elems, const float* scale,
                             const float* shift, int relu, void* dst, int dst_channels_total, int dst_channel_offset, int dst_layout,
                             long long dst_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool two = channels1 != 0;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "neck_conv_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(height0 >= 1 && width0 >= 1 && out_height >= 1 && out_width >= 1 && (!two || (height1 >= 1 && width1 >= 1)),
                 "neck_conv_forward: bad sizes (maps %d x %d and %d x %d, output %d x %d)", height0, width0, height1, width1, out_height,
                 out_width);
  BEVAMD_REQUIRE((layout0 == 0 || layout0 == 1) && (!two || layout1 == 0 || layout1 == 1) && (dst_layout == 0 || dst_layout == 1),
                 "neck_conv_forward: layouts are 0 (NCHW) or 1 (NHWC), got %d, %d and %d", layout0, layout1, dst_layout);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "neck_conv_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  if (kernel != 1 && kernel != 3) {
    set_error("neck_conv_forward: not supported (kernel %d; 1 or 3, stride 1, padding kernel / 2)", kernel);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (channels0 < 16 || channels0 % 16 || channels1 < 0 || channels1 % 16 || out_channels < 32 || out_channels % 32) {
    set_error("neck_conv_forward: not supported (source channels %d and %d must be multiples of 16, out_channels %d a multiple of 32)",
              channels0, channels1, out_channels);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (dst_layout == 1 && (dst_channels_total % 4 || dst_channel_offset % 4)) {
    set_error("neck_conv_forward: not supported (an NHWC destination needs dst_channels_total %d and dst_channel_offset %d in multiples of 4)",
              dst_channels_total, dst_channel_offset);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(dst_channel_offset >= 0 && (long long)dst_channel_offset + out_channels <= dst_channels_total,
                 "neck_conv_forward: the window [%d, %d + %d) does not fit %d destination channels", dst_channel_offset, dst_channel_offset,
                 out_channels, dst_channels_total);
  BEVAMD_REQUIRE((long long)height0 * width0 <= 0x7fffffffLL && (!two || (long long)height1 * width1 <= 0x7fffffffLL),
                 "neck_conv_forward: a source map has more than 2^31 - 1 pixels");
  const int nch = (int)(((long long)channels0 + channels1 + CK - 1) / CK);
  const long long want_packed = (long long)out_channels * nch * kernel * kernel * CK;
  BEVAMD_REQUIRE(packed_elems == want_packed, "neck_conv_forward: packed holds %lld elements, this layer needs %lld", packed_elems, want_packed);
  const long long want_dst = (long long)batch * dst_channels_total * out_height * (long long)out_width;
  BEVAMD_REQUIRE(dst_elems == want_dst, "neck_conv_forward: dst holds %lld elements, [%d, %d, %d, %d] needs %lld", dst_elems, batch,
                 dst_channels_total, out_height, out_width, want_dst);
  const long long tiles_x = cdiv(out_width, NK_TW), tiles = tiles_x * cdiv(out_height, NK_TH);
  BEVAMD_REQUIRE(tiles <= 0x7fffffffLL, "neck_conv_forward: a %d x %d map has too many tiles", out_height, out_width);
  BEVAMD_REQUIRE(packed != nullptr && ((uintptr_t)packed & 15) == 0, "neck_conv_forward: packed is null or not 16-byte aligned");
  BEVAMD_REQUIRE(scale != nullptr && shift != nullptr && (((uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
                 "neck_conv_forward: scale or shift is null or not 16-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(src0 != nullptr && dst != nullptr && (!two || src1 != nullptr), "neck_conv_forward: a source or dst is null");
  BEVAMD_REQUIRE((layout0 == 0 || ((uintptr_t)src0 & 15) == 0) && (!two || layout1 == 0 || ((uintptr_t)src1 & 15) == 0),
                 "neck_conv_forward: an NHWC source is not 16-byte aligned");
  BEVAMD_REQUIRE(dst_layout == 0 || ((uintptr_t)dst & 7) == 0, "neck_conv_forward: an NHWC dst is not 8-byte aligned");

  auto ratio = [](int n, int N) { return N > 1 ? (float)(n - 1) / (float)(N - 1) : 0.f; };
  NkArgs a;
  a.src0 = (const unsigned short*)src0;
  a.src1 = two ? (const unsigned short*)src1 : nullptr;
  a.c0 = channels0;
  a.c1 = channels1;
  a.h0 = height0;
  a.w0 = width0;
  a.h1 = two ? height1 : 1;
  a.w1 = two ? width1 : 1;
  a.nhwc0 = layout0;
  a.nhwc1 = two ? layout1 : 0;
  a.rs0 = height0 != out_height || width0 != out_width;
  a.rs1 = two && (height1 != out_height || width1 != out_width);
  a.ry0 = ratio(a.h0, out_height);
  a.rx0 = ratio(a.w0, out_width);
  a.ry1 = ratio(a.h1, out_height);
  a.rx1 = ratio(a.w1, out_width);
  a.OH = out_height;
  a.OW = out_width;
  a.cout = out_channels;
  a.nch = nch;
  a.tiles_x = (int)tiles_x;
  a.relu = relu != 0;
  a.packed = (const unsigned short*)packed;
  a.scale = scale;
  a.shift = shift;
  a.dst = (unsigned short*)dst;
  a.dst_c = dst_channels_total;
  a.dst_off = dst_channel_offset;
  a.dst_nhwc = dst_layout;
  if (dtype == 1) nk_dispatch<true>(a, kernel, batch, stream);
  else nk_dispatch<false>(a, kernel, batch, stream);
  BEVAMD_LAUNCH_CHECK("cam_neck_conv");
  return BEVAMD_OK;
}

}  // extern "C"
