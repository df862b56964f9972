// The stem of a ResNet in eval mode, gfx950: conv 7x7 stride 2 (3 -> 64) + folded BatchNorm + ReLU + MaxPool 3x3 stride 2 in ONE
// launch.
//
// Replaces (mmdet 2.x mmdet/models/backbones/resnet.py, ResNet.forward):
//     x = self.conv1(x);  x = self.norm1(x);  x = self.relu(x);  x = self.maxpool(x)
//   four launches, the 64-channel half-resolution map written and read three times to produce a map a quarter its size.
//
// Native formulation: implicit GEMM D[channel][conv pixel] with the MFMA, the fragment layouts and the epilogue pieces of
// dense_tile.h, its own staging and B operand; the conv map never reaches memory.
//   * A workgroup of four waves owns 4 x 15 pooled pixels x 64 channels of one image.  They need the 9 x 31 conv pixels from
//     (2 ph0 - 1, 2 pw0 - 1); the workgroup computes 9 x 32 (18 MFMA column tiles of 16 conv pixels of one conv row, dealt to the
//     waves round robin) from the 23 x 70 x 3 input tile from (4 ph0 - 5, 4 pw0 - 5), staged once in LDS as [ci][row][72] with
//     zeros outside the image.
//   * K order: k = 8 pair + kx with pair = 7 ci + ky (21 pairs padded to 24) and kx padded from 7 to 8: K = 192, six k-steps of 32.
//     A lane's B fragment (k = 8 (lane >> 4) + j) is the 8 consecutive input pixels 2 cx .. 2 cx + 7 of LDS row (ci, 2 cy + ky); the
//     eighth pixel and the padding pairs are cleared in the fragment, so nothing outside the 7 x 7 window is multiplied.  The
//     weights come packed in that order (stem_pack_weight: zero at kx = 7 and pair >= 21) and stay in registers: 24 fragments.
//   * Epilogue, fp32, no contraction: v = max(fma(acc, scale, shift), 0), rounded ONCE to 16 bits into the LDS conv tile
//     [pixel][64 + 4].  After a barrier a thread pools 8 channels of one pooled pixel over the window's cells inside the conv map.
//     Rounding is monotone, so the maximum of the rounded values IS the rounded maximum of the fp32 values.
// Every conv value is ONE accumulator chain in ascending k: no atomics, no split-K; equal calls give equal bits and a sample's
// result does not depend on the batch around it.
#include "dense_tile.h"

namespace bevamd {

constexpr int ST_TPH = 4, ST_TPW = 15;                        // pooled pixels of one workgroup
constexpr int ST_CH = 2 * ST_TPH + 1, ST_CW = 32;             // conv pixels it computes (31 columns are pooled)
constexpr int ST_IH = 2 * (ST_CH - 1) + 7;                    // 23 input rows
constexpr int ST_IW = 2 * (ST_CW - 1) + 8;                    // 70 input columns (the eighth tap column included)
constexpr int ST_RS = 72;                                     // 16-bit elements per input row in LDS
constexpr int ST_CSTR = 64 + 4;                               // 16-bit elements per conv pixel in LDS
constexpr int ST_THREADS = 256;
constexpr int ST_KSTEPS = 6, ST_PAIRS = 21;
constexpr int ST_TILES = ST_CH * (ST_CW / 16);                // MFMA column tiles of one workgroup
constexpr int ST_IN_ELEMS = 3 * ST_IH * ST_RS;
constexpr int ST_PACKED = 4 * ST_KSTEPS * 64 * 8;             // elements of the packed weight
static_assert(2 * ST_TPW + 1 <= ST_CW && ST_IW <= ST_RS && ST_RS % 2 == 0, "the pooled tile's windows lie inside the conv tile");

struct StArgs {
  const unsigned short* x;
  int H, W, OH, OW, PH, PW;
  int tiles_x;
  const unsigned short* packed;
  const float* scale;
  const float* shift;
  unsigned short* dst;
  int dst_nhwc;
};

template <bool BF16>
__global__ __launch_bounds__(ST_THREADS) void resnet_stem_kernel(StArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short in_s[ST_IN_ELEMS];
  __shared__ __attribute__((aligned(16))) unsigned short conv_s[ST_CH * ST_CW * ST_CSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int b = blockIdx.z;
  const int ph0 = ty * ST_TPH, pw0 = tx * ST_TPW;
  const int cy0 = 2 * ph0 - 1, cx0 = 2 * pw0 - 1;            // the conv tile's first pixel
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;            // the input tile's first pixel

  // the input tile, zero outside the image
  {
    const size_t hw = (size_t)a.H * a.W;
    const unsigned short* xb = a.x + (size_t)b * 3 * hw;
#pragma unroll 1
    for (int idx = tid; idx < ST_IN_ELEMS; idx += ST_THREADS) {
      const int ci = idx / (ST_IH * ST_RS), rem = idx - ci * (ST_IH * ST_RS);
      const int iy = rem / ST_RS, ix = rem - iy * ST_RS;
      const int gy = iy0 + iy, gx = ix0 + ix;
      unsigned short v = 0;
      if (ix < ST_IW && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = xb[(size_t)ci * hw + (size_t)gy * a.W + gx];
      in_s[idx] = v;
    }
  }

  const int lr = lane & 15, lg = lane >> 4;
  // A fragments: [mt][kstep][lane] units of 16 bytes, all 24 in registers
  u32x4 af[4][ST_KSTEPS];
  {
    const u32x4* wp = reinterpret_cast<const u32x4*>(a.packed) + lane;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int ks = 0; ks < ST_KSTEPS; ++ks) af[m][ks] = wp[(m * ST_KSTEPS + ks) * 64];
  }
  // the lane's LDS row of k-step ks: pair = 4 ks + lg = 7 ci + ky
  int rowoff[ST_KSTEPS];
  bool pair_live[ST_KSTEPS];
#pragma unroll
  for (int ks = 0; ks < ST_KSTEPS; ++ks) {
    const int pair = 4 * ks + lg;
    pair_live[ks] = pair < ST_PAIRS;
    const int pc = pair_live[ks] ? pair : 0;
    const int ci = pc / 7, ky = pc - 7 * ci;
    rowoff[ks] = (ci * ST_IH + ky) * ST_RS;
  }
  Affine4 bn[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) bn[m] = load_affine4(a.scale, a.shift, 16 * m + 4 * lg);
  __syncthreads();

#pragma unroll 1
  for (int t = wave; t < ST_TILES; t += 4) {
    const int r = t >> 1, c = (t & 1) * 16 + lr;             // the lane's conv pixel of the tile
    const unsigned short* src = in_s + (2 * r) * ST_RS + 2 * c;
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < ST_KSTEPS; ++ks) {
      const unsigned int* q = reinterpret_cast<const unsigned int*>(src + rowoff[ks]);
      u32x4 bf;
      bf[0] = q[0];
      bf[1] = q[1];
      bf[2] = q[2];
      bf[3] = q[3] & 0xffffu;                                // the eighth pixel is outside the 7 x 7 window
      if (!pair_live[ks]) bf = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = mfma16<BF16>(af[m][ks], bf, acc[m]);
    }
    // D fragment: pixel on the lane (lr), channel = 16 m + 4 lg + reg
    unsigned short* d = conv_s + (r * ST_CW + c) * ST_CSTR + 4 * lg;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      unsigned short v[4];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) v[q4] = round16<BF16>(relu(affine(acc[m][q4], bn[m], q4)));
      *reinterpret_cast<u32x2*>(d + 16 * m) = pack4(v[0], v[1], v[2], v[3]);
    }
  }
  __syncthreads();

  // pooling: a unit is 8 channels of one pooled pixel
  constexpr int UNITS = ST_TPH * ST_TPW * 8;
  const size_t phw = (size_t)a.PH * a.PW;
#pragma unroll 1
  for (int idx = tid; idx < UNITS; idx += ST_THREADS) {
    int g, p;
    if (a.dst_nhwc) { g = idx & 7; p = idx >> 3; } else { g = idx / (ST_TPH * ST_TPW); p = idx - g * (ST_TPH * ST_TPW); }
    const int i = p / ST_TPW, j = p - i * ST_TPW;
    const int ph = ph0 + i, pw = pw0 + j;
    if (ph >= a.PH || pw >= a.PW) continue;
    float best[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool any = false;                                                  // the window's centre (2 ph, 2 pw) is always in the map
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int r = 2 * i + dy, c = 2 * j + dx;
        const int cy = cy0 + r, cx = cx0 + c;
        if (cy < 0 || cy >= a.OH || cx < 0 || cx >= a.OW) continue;     // cells outside the conv map do not take part
        const u32x4 w = *reinterpret_cast<const u32x4*>(conv_s + (r * ST_CW + c) * ST_CSTR + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = widen16<BF16>((unsigned short)(w[e] & 0xffffu)), hi = widen16<BF16>((unsigned short)(w[e] >> 16));
          best[2 * e] = any ? fmaxf(best[2 * e], lo) : lo;
          best[2 * e + 1] = any ? fmaxf(best[2 * e + 1], hi) : hi;
        }
        any = true;
      }
    }
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = round16<BF16>(best[e]);          // exact: the values are 16-bit already
    if (a.dst_nhwc) {
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (unsigned int)v[2 * e] | ((unsigned int)v[2 * e + 1] << 16);
      *reinterpret_cast<u32x4*>(a.dst + (((size_t)b * a.PH + ph) * a.PW + pw) * 64 + 8 * g) = o;
    } else {
      unsigned short* d = a.dst + ((size_t)b * 64 + 8 * g) * phw + (size_t)ph * a.PW + pw;
#pragma unroll
      for (int e = 0; e < 8; ++e) d[(size_t)e * phw] = v[e];
    }
  }
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_resnet_stem_forward(const void* x, int dtype, int batch, int in_channels, int height, int width, int out_channels,
                               int kernel, int stride, int padding, int pool_kernel, int pool_stride, int pool_padding,
                               int pool_ceil_mode, const void* packed, long long packed_elems, const float* scale,
                               const float* shift, void* dst, int dst_layout, long long dst_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "resnet_stem_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(height >= 1 && width >= 1, "resnet_stem_forward: bad sizes (image %d x %d)", height, width);
  BEVAMD_REQUIRE(dst_layout == 0 || dst_layout == 1, "resnet_stem_forward: dst_layout is 0 (NCHW) or 1 (NHWC), got %d", dst_layout);
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "resnet_stem_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  if (in_channels != 3 || out_channels != 64 || kernel != 7 || stride != 2 || padding != 3) {
    set_error("resnet_stem_forward: not supported (convolution %d -> %d, kernel %d, stride %d, padding %d; served: 3 -> 64, 7, 2, 3)",
              in_channels, out_channels, kernel, stride, padding);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (pool_kernel != 3 || pool_stride != 2 || pool_padding != 1 || pool_ceil_mode != 0) {
    set_error("resnet_stem_forward: not supported (pooling kernel %d, stride %d, padding %d, ceil_mode %d; served: 3, 2, 1, 0)",
              pool_kernel, pool_stride, pool_padding, pool_ceil_mode);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  const int OH = (height - 1) / 2 + 1, OW = (width - 1) / 2 + 1;
  const int PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1;
  BEVAMD_REQUIRE(packed_elems == ST_PACKED, "resnet_stem_forward: packed holds %lld elements, the stem needs %d", packed_elems, ST_PACKED);
  const long long want_dst = (long long)batch * 64 * PH * (long long)PW;
  BEVAMD_REQUIRE(dst_elems == want_dst, "resnet_stem_forward: dst holds %lld elements, [%d, 64, %d, %d] needs %lld", dst_elems, batch,
                 PH, PW, want_dst);
  const long long tiles_x = cdiv(PW, ST_TPW), tiles = tiles_x * cdiv(PH, ST_TPH);
  BEVAMD_REQUIRE(tiles <= 0x7fffffffLL && (long long)height * width <= 0x7fffffffLL,
                 "resnet_stem_forward: a %d x %d image has too many tiles", height, width);
  BEVAMD_REQUIRE(packed != nullptr && ((uintptr_t)packed & 15) == 0, "resnet_stem_forward: packed is null or not 16-byte aligned");
  BEVAMD_REQUIRE(scale != nullptr && shift != nullptr && (((uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
                 "resnet_stem_forward: scale or shift is null or not 16-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(x != nullptr && dst != nullptr, "resnet_stem_forward: x or dst is null");
  BEVAMD_REQUIRE((((uintptr_t)x | (uintptr_t)dst) & 1) == 0, "resnet_stem_forward: x or dst is not 2-byte aligned");
  BEVAMD_REQUIRE(dst_layout == 0 || ((uintptr_t)dst & 15) == 0, "resnet_stem_forward: an NHWC dst is not 16-byte aligned");
  const long long x_bytes = 2LL * batch * 3 * height * (long long)width;
  BEVAMD_REQUIRE(!ranges_overlap(dst, 2 * want_dst, x, x_bytes), "resnet_stem_forward: dst overlaps x");

  StArgs a;
  a.x = (const unsigned short*)x;
  a.H = height;
  a.W = width;
  a.OH = OH;
  a.OW = OW;
  a.PH = PH;
  a.PW = PW;
  a.tiles_x = (int)tiles_x;
  a.packed = (const unsigned short*)packed;
  a.scale = scale;
  a.shift = shift;
  a.dst = (unsigned short*)dst;
  a.dst_nhwc = dst_layout;
  if (dtype == 1)
    resnet_stem_kernel<true><<<dim3((unsigned)tiles, 1, batch), dim3(ST_THREADS), 0, stream>>>(a);
  else
    resnet_stem_kernel<false><<<dim3((unsigned)tiles, 1, batch), dim3(ST_THREADS), 0, stream>>>(a);
  BEVAMD_LAUNCH_CHECK("resnet_stem");
  return BEVAMD_OK;
}

}  // extern "C"
