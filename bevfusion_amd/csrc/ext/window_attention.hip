// Shifted-window multi-head attention of a Swin block in eval mode, gfx950: ONE launch from the qkv map to the output map.
//
// Replaces (mmdet 2.x mmdet/models/backbones/swin.py, the camera backbone `SwinTransformer`): ShiftWindowMSA.forward + WindowMSA.forward
// between the qkv Linear and the proj Linear: pad, roll, window partition, reshape / permute of qkv, q * scale, q @ k^T, the relative
// position bias, the shift mask, softmax, attn @ v, window reverse, roll back, crop: about fifteen launches, and the
// [windows * B, heads, 49, 49] logits written and read several times.
//
// Native formulation.  No rolled, partitioned or padded tensor exists: token (ty, tx) of window (wy, wx) IS pixel
// y = (7 wy + ty + shift) mod Hp, x = (7 wx + tx + shift) mod Wp of the qkv map (Hp, Wp: the sizes rounded up to 7), or the padded
// token pad_qkv when that pixel lies outside the map; the output goes back to the same pixel, so reverse, roll back and crop are free.
//   * One wave owns one (window, head): 49 tokens padded to 64 = four MFMA tiles, head dimension 32 = one k-step of
//     v_mfma_f32_16x16x32.  A workgroup is four waves: four consecutive windows of ONE head, which share that head's bias in LDS.
//   * S^T = K Q^T (16 MFMAs): A = K [key 16 kt + (lane & 15)][d = 8 (lane >> 4) + j], B = Q [d][query 16 qt + (lane & 15)], both one
//     16-byte load per lane and tile straight from the map (no LDS).  D puts the QUERY on the lane (lane & 15) and the keys
//     16 kt + 4 (lane >> 4) + reg in registers and lane groups, so the softmax of a row is 16 values in-lane plus two cross-group steps.
//   * logit = fma(S, scale, bias) + mask in fp32; the mask is arithmetic: region(r) = 0 if r < Hp - 7, 1 if r < Hp - shift, else 2 of
//     the ROLLED row r = 7 wy + ty, columns alike; -100 where (row region, column region) of query and key differ.  Maximum, exp and
//     the row sum are fp32; the 15 padding keys get p = 0.
//   * O^T = V^T P^T (16 MFMAs).  P goes DIRECTLY from the accumulators into the B operand: the k-step s takes the key tiles 2 s and
//     2 s + 1, slot 8 (lane >> 4) + j of the step is key 16 (2 s + (j >> 2)) + 4 (lane >> 4) + (j & 3), which is what the lane already
//     holds for its query; P is rounded once to the storage type.  V is staged in LDS TRANSPOSED and in that same key order
//     (vt[d][slot], 4.5 KiB per wave), so its A fragment [d = 16 dt + (lane & 15)][8 slots] is one 16-byte LDS read.
//   * D of the second product: query on the lane, d = 16 dt + 4 (lane >> 4) + reg: four channels of one pixel are normalised by the
//     lane's own fp32 row sum, rounded once, and stored as 8 bytes.
// No atomics, no workspace, no scratch: equal calls give equal bits and a sample's result does not depend on the batch around it.
#include "dense_tile.h"

namespace bevamd {

constexpr int WA_WS = 7;                         // window side
constexpr int WA_N = WA_WS * WA_WS;              // tokens of a window
constexpr int WA_HD = 32;                        // head dimension
constexpr int WA_WAVES = 4;                      // (window, head) pairs of one workgroup
constexpr int WA_THREADS = 64 * WA_WAVES;
constexpr int WA_VSTR = 64 + 8;                  // 16-bit elements per row of vt (144 bytes: 16-byte aligned rows, spread banks)
constexpr int WA_BIAS = WA_N * WA_N;             // floats of one head's bias
constexpr int WA_BIAS_BYTES = (WA_BIAS * 4 + 15) / 16 * 16;
constexpr int WA_VT_BYTES = WA_HD * WA_VSTR * 2;

struct WaArgs {
  const unsigned short* qkv;
  const unsigned short* pad;                     // [3C] or null (zeros)
  const float* bias;
  unsigned short* out;
  int H, W, C;
  int Hp, Wp, nwx, per;                          // padded sizes, windows per row and per sample
  long long nwin;                                // batch * per
  int shift;
  float scale;
};

struct WaToken {
  const unsigned short* src;                     // channel 0 of the token's qkv (the map, or pad); null: all zeros
  long long pix;                                 // its pixel b * H * W + y * W + x, -1 where nothing is written
  int region;                                    // 3 * row region + column region of the rolled frame (0 without a shift)
};

__device__ __forceinline__ int wa_region(const WaArgs& a, int wy, int wx, int t) {
  if (a.shift == 0 || t >= WA_N) return 0;
  const int ty = t / WA_WS, tx = t - ty * WA_WS;
  const int r = WA_WS * wy + ty, c = WA_WS * wx + tx;
  const int rr = r < a.Hp - WA_WS ? 0 : (r < a.Hp - a.shift ? 1 : 2);
  const int cr = c < a.Wp - WA_WS ? 0 : (c < a.Wp - a.shift ? 1 : 2);
  return 3 * rr + cr;
}

__device__ __forceinline__ WaToken wa_token(const WaArgs& a, int b, int wy, int wx, int t) {
  WaToken k;
  k.src = nullptr;
  k.pix = -1;
  k.region = wa_region(a, wy, wx, t);
  if (t >= WA_N) return k;
  const int ty = t / WA_WS, tx = t - ty * WA_WS;
  int y = WA_WS * wy + ty + a.shift, x = WA_WS * wx + tx + a.shift;
  if (y >= a.Hp) y -= a.Hp;
  if (x >= a.Wp) x -= a.Wp;
  if (y < a.H && x < a.W) {
    k.pix = ((long long)b * a.H + y) * a.W + x;
    k.src = a.qkv + (size_t)k.pix * (size_t)(3 * a.C);
  } else {
    k.src = a.pad;
  }
  return k;
}

// 8 channels from `off` of a token as one 16-byte unit
__device__ __forceinline__ u32x4 wa_load(const unsigned short* src, int off) {
  if (src == nullptr) return u32x4{0u, 0u, 0u, 0u};
  return *reinterpret_cast<const u32x4*>(src + off);
}

// the slot of key k in the k-steps of the second product (see the head of the file)
__device__ __forceinline__ int wa_slot(int k) { return 32 * (k >> 5) + 8 * ((k >> 2) & 3) + 4 * ((k >> 4) & 1) + (k & 3); }

template <bool BF16>
__global__ __launch_bounds__(WA_THREADS, 4) void window_attention_kernel(WaArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[WA_BIAS_BYTES + WA_WAVES * WA_VT_BYTES];
  float* bias_s = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int head = blockIdx.y;
  unsigned short* vt = reinterpret_cast<unsigned short*>(smem + WA_BIAS_BYTES + wave * WA_VT_BYTES);

  {
    const float* bsrc = a.bias + (size_t)head * WA_BIAS;
    for (int i = tid; i < WA_BIAS; i += WA_THREADS) bias_s[i] = bsrc[i];
  }

  const long long win = (long long)blockIdx.x * WA_WAVES + wave;
  const bool live = win < a.nwin;                // wave-uniform
  int b = 0, wy = 0, wx = 0;
  WaToken tk[4];
  u32x4 qf[4], kf[4];
  if (live) {
    b = (int)(win / a.per);
    const int rem = (int)(win - (long long)b * a.per);
    wy = rem / a.nwx;
    wx = rem - wy * a.nwx;
    const int qoff = head * WA_HD + lg * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      tk[t] = wa_token(a, b, wy, wx, 16 * t + lr);
      qf[t] = wa_load(tk[t].src, qoff);
      kf[t] = wa_load(tk[t].src, a.C + qoff);
    }
    // V, transposed and in slot order: a unit is the 8 channels 8 g .. of the key pair (2 p, 2 p + 1), which are neighbouring slots
    const int voff = 2 * a.C + head * WA_HD;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = lane + 64 * i;
      const int p = u >> 2, g = u & 3;
      const WaToken t0 = wa_token(a, b, wy, wx, 2 * p), t1 = wa_token(a, b, wy, wx, 2 * p + 1);
      const u32x4 v0 = wa_load(t0.src, voff + 8 * g), v1 = wa_load(t1.src, voff + 8 * g);
      unsigned int* dst = reinterpret_cast<unsigned int*>(vt + (8 * g) * WA_VSTR + wa_slot(2 * p));
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned int h0 = (v0[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        const unsigned int h1 = (v1[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        dst[e * (WA_VSTR / 2)] = h0 | (h1 << 16);
      }
    }
  }
  __syncthreads();
  if (!live) return;

  // S^T: s[kt][qt][reg] = K[key 16 kt + 4 lg + reg] . Q[query 16 qt + lr]
  f32x4 s[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) s[kt][qt] = mfma16<BF16>(kf[kt], qf[qt], f32x4{0.f, 0.f, 0.f, 0.f});

  // the regions of the lane's 16 keys, four bits each
  unsigned long long kreg = 0ull;
  if (a.shift > 0) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        kreg |= (unsigned long long)wa_region(a, wy, wx, 16 * kt + 4 * lg + r) << (4 * (4 * kt + r));
  }

  float inv[4];
  u32x4 pf[2][4];                                 // B fragments of P: [k-step][query tile]
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) {
    const int q = 16 * qt + lr;
    const int qrow = (q < WA_N ? q : WA_N - 1) * WA_N;      // queries 49 .. 63 compute a finite row that is never stored
    const int qreg = tk[qt].region;
    float l[4][4];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + 4 * lg + r;
        float v = -INFINITY;
        if (key < WA_N) {
          v = fmaf(s[kt][qt][r], a.scale, bias_s[qrow + key]);
          if ((int)((kreg >> (4 * (4 * kt + r))) & 15ull) != qreg) v += -100.f;
        }
        l[kt][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + 4 * lg + r;
        const float p = key < WA_N ? __expf(l[kt][r] - mx) : 0.f;
        l[kt][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    inv[qt] = 1.f / sum;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      unsigned int h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = round16<BF16>(l[2 * st + (j >> 2)][j & 3]);
      pf[st][qt] = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    }
  }

  // O^T: o[dt][qt][reg] = sum_key V[key][d = 16 dt + 4 lg + reg] P[query 16 qt + lr][key]
  f32x4 o[2][4];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) o[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < 2; ++st)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const u32x4 vf = *reinterpret_cast<const u32x4*>(vt + (16 * dt + lr) * WA_VSTR + 32 * st + 8 * lg);
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) o[dt][qt] = mfma16<BF16>(vf, pf[st][qt], o[dt][qt]);
    }

#pragma unroll
  for (int qt = 0; qt < 4; ++qt) {
    if (tk[qt].pix < 0) continue;
    unsigned short* dst = a.out + (size_t)tk[qt].pix * (size_t)a.C + head * WA_HD + 4 * lg;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      unsigned short r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = round16<BF16>(o[dt][qt][e] * inv[qt]);
      *reinterpret_cast<u32x2*>(dst + 16 * dt) = pack4(r[0], r[1], r[2], r[3]);
    }
  }
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_window_attention_forward(const void* qkv, long long qkv_elems, const void* pad_qkv, long long pad_elems, const float* bias,
                                    long long bias_elems, int dtype, int batch, int height, int width, int channels, int heads,
                                    int window, int head_dim, float scale, int shift, void* out, long long out_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (window != WA_WS || head_dim != WA_HD) {
    set_error("window_attention_forward: not supported (window %d, head dimension %d; the kernel is built for 7 and 32)", window,
              head_dim);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "window_attention_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  BEVAMD_REQUIRE(batch >= 0 && height >= 1 && width >= 1, "window_attention_forward: bad sizes (batch %d, map %d x %d)", batch, height,
                 width);
  BEVAMD_REQUIRE(heads >= 1 && heads <= 65535 && channels == heads * WA_HD,
                 "window_attention_forward: %d channels are not %d heads of %d (1 .. 65535 heads)", channels, heads, WA_HD);
  BEVAMD_REQUIRE(shift >= 0 && shift < WA_WS, "window_attention_forward: shift %d (0 .. 6)", shift);
  BEVAMD_REQUIRE(scale == scale && scale - scale == 0.f, "window_attention_forward: scale is not finite");
  const long long pixels = (long long)batch * height * (long long)width;
  BEVAMD_REQUIRE(height <= (1 << 24) && width <= (1 << 24) && pixels <= (1LL << 40), "window_attention_forward: a %d x %d x %d map is too large",
                 batch, height, width);
  const long long want_qkv = pixels * 3 * channels, want_out = pixels * channels, want_bias = (long long)heads * WA_BIAS;
  BEVAMD_REQUIRE(qkv_elems == want_qkv, "window_attention_forward: qkv holds %lld elements, [%d, %d, %d, %d] needs %lld", qkv_elems,
                 batch, height, width, 3 * channels, want_qkv);
  BEVAMD_REQUIRE(out_elems == want_out, "window_attention_forward: out holds %lld elements, [%d, %d, %d, %d] needs %lld", out_elems,
                 batch, height, width, channels, want_out);
  BEVAMD_REQUIRE(bias_elems == want_bias, "window_attention_forward: bias holds %lld floats, [%d, 49, 49] needs %lld", bias_elems, heads,
                 want_bias);
  BEVAMD_REQUIRE(pad_qkv == nullptr ? pad_elems == 0 : pad_elems == 3LL * channels,
                 "window_attention_forward: pad_qkv holds %lld elements, needs %lld (0 when null)", pad_elems, 3LL * channels);
  BEVAMD_REQUIRE(bias != nullptr && ((uintptr_t)bias & 3) == 0, "window_attention_forward: bias is null or not 4-byte aligned");
  BEVAMD_REQUIRE(((uintptr_t)pad_qkv & 15) == 0, "window_attention_forward: pad_qkv is not 16-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(qkv != nullptr && out != nullptr, "window_attention_forward: qkv or out is null");
  BEVAMD_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 7) == 0,
                 "window_attention_forward: qkv is not 16-byte aligned or out not 8-byte aligned");
  BEVAMD_REQUIRE(!ranges_overlap(out, 2 * want_out, qkv, 2 * want_qkv), "window_attention_forward: out overlaps qkv");
  BEVAMD_REQUIRE(pad_qkv == nullptr || !ranges_overlap(out, 2 * want_out, pad_qkv, 6LL * channels),
                 "window_attention_forward: out overlaps pad_qkv");
  BEVAMD_REQUIRE(!ranges_overlap(out, 2 * want_out, bias, 4 * want_bias), "window_attention_forward: out overlaps bias");

  WaArgs a;
  a.qkv = (const unsigned short*)qkv;
  a.pad = (const unsigned short*)pad_qkv;
  a.bias = bias;
  a.out = (unsigned short*)out;
  a.H = height;
  a.W = width;
  a.C = channels;
  const int nwy = (height + WA_WS - 1) / WA_WS;
  a.nwx = (width + WA_WS - 1) / WA_WS;
  a.Hp = nwy * WA_WS;
  a.Wp = a.nwx * WA_WS;
  const long long per = (long long)nwy * a.nwx;
  a.nwin = per * batch;
  const long long groups = (a.nwin + WA_WAVES - 1) / WA_WAVES;
  BEVAMD_REQUIRE(per <= 0x7fffffffLL && groups <= 0x7fffffffLL, "window_attention_forward: a %d x %d x %d map has too many windows", batch,
                 height, width);
  a.per = (int)per;
  a.shift = shift;
  a.scale = scale;
  const dim3 grid((unsigned)groups, (unsigned)heads, 1);
  if (dtype == 1)
    window_attention_kernel<true><<<grid, dim3(WA_THREADS), 0, stream>>>(a);
  else
    window_attention_kernel<false><<<grid, dim3(WA_THREADS), 0, stream>>>(a);
  BEVAMD_LAUNCH_CHECK("window_attention");
  return BEVAMD_OK;
}

}  // extern "C"
