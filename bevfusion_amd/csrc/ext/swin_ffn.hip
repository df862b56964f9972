// The FFN half of a Swin block in eval mode, gfx950: LayerNorm, fc1, GELU, fc2 and the residual in ONE launch.
//
// Replaces (mmdet 2.x mmdet/models/backbones/swin.py SwinBlock.forward, `self.ffn(self.norm2(x), identity=x)` over mmcv's FFN):
// nn.LayerNorm, Linear C -> hidden, nn.GELU (the erf form), Linear hidden -> C, add: five launches, and the [tokens, hidden]
// activations written by fc1, read and written by GELU and read by fc2.  Here they never leave the registers.
//
// Per token row x[t, 0 .. C), in fp32 without contraction:
//   mean = (sum_c x_c) / C        var = (sum_c (x_c - mean)^2) / C        rstd = 1 / sqrt(var + eps)          (two passes, c ascending)
//   n_c  = round16(fma((x_c - mean) * rstd, gamma_c, beta_c))
//   h_j  = round16(gelu(sum_c W1[j][c] n_c + b1_j))      gelu(t) = 0.5 t (1 + erf(t / sqrt 2))
//   out_c = round16(x_c + (sum_j W2[c][j] h_j + b2_c))
// Three roundings.  Both sums are ONE accumulator chain on v_mfma_f32_16x16x32: the first in ascending c, the second in ascending
// k-step of 32 hidden units, inside a step in the MFMA's own order.  No split-K, no atomics, no workspace.
//
// Tile.  One wave (= one workgroup of 64 threads) owns 32 tokens = two MFMA token tiles, and ALL C output channels of them: C / 2
// accumulator registers a lane, so two waves share a SIMD at every width up to 192.  (64 tokens a wave halve the weight traffic
// through L2 but leave one wave per SIMD above 96 channels, and measured slower at every shape: profiles/EXPERIMENTS.md.)
//   * Staging: the 32 x C tile of x goes to LDS as [token][C + 8] in 16-byte units, consecutive lanes reading consecutive units;
//     rows past the last token are zero and no address past row T - 1 is formed.
//   * LayerNorm: lane t < 32 holds row t in registers (C / 8 LDS reads of 16 bytes; the row stride of (C + 8) / 2 dwords is 4 mod 16,
//     which spreads the 16 lanes of a read group over all banks), takes both passes in-lane and writes n back over its own row.
//   * Both products put the weights on A and the tokens on B, so D has the TOKEN on the lane (lane & 15) and the output unit in
//     registers and lane groups: unit 16 tile + 4 (lane >> 4) + reg.
//   * The hidden units are walked in k-steps s of 32 = two MFMA tiles 2 s, 2 s + 1.  h^T = W1 n^T: A = W1 [j = 16 tile + (lane & 15)]
//     [c = 32 ks + 8 (lane >> 4) + e], B = n [c][token 16 tt + (lane & 15)] = one 16-byte LDS read.  After bias, GELU and rounding
//     the lane holds, for each of its two tokens, the hidden units 32 s + 16 (e >> 2) + 4 (lane >> 4) + (e & 3), e = 0 .. 7: these
//     eight ARE its B fragment of k-step s of the second product, out^T += W2 h^T, when W2's k-step is packed in that same order.
//     No LDS round trip for h.
//   * W1 and W2 stream from L2 once per wave (32 tokens per pass over the 16 C^2 bytes): W2 of step s and W1 of step s + 1 are
//     requested right after the first product of step s, so both loads fly under the step's GELU.
//   * Epilogue: four channels of one token: x again (8 bytes, a cache hit), + (acc + b2), one rounding, an 8-byte store.
//
// Packed operands (what the host builds, see cam_swin.fold_swin_ffn), 16-bit elements, KS = C / 32, CT = C / 16:
//   packed1[((tile * KS + ks) * 64 + lane) * 8 + e] = W1[16 tile + (lane & 15)][32 ks + 8 (lane >> 4) + e]         tile < hidden / 16
//   packed2[((s * CT + ct) * 64 + lane) * 8 + e]    = W2[16 ct + (lane & 15)][32 s + 16 (e >> 2) + 4 (lane >> 4) + (e & 3)]   s < hidden / 32
//
// Equal calls give equal bits, and a token's result depends on its own row alone (the tile it falls into changes nothing: every
// token has its own lane slot in B and D).
#include <cmath>

#include "dense_tile.h"

namespace bevamd {

constexpr int SF_NT = 2;                         // MFMA token tiles of one wave (profiles/EXPERIMENTS.md has the sweep over 1, 2, 4)
constexpr int SF_TOK = 16 * SF_NT;               // tokens of one wave
constexpr int SF_CMAX = 192;                     // widest token the kernel is built for
constexpr int SF_HMAX = 4 * SF_CMAX;

struct SfArgs {
  const unsigned short* x;
  const float *gamma, *beta, *b1, *b2;
  const u32x4 *w1, *w2;
  unsigned short* out;
  long long T;
  int hidden;
  float eps;
};

// gelu(t) = 0.5 t (1 + erf(z)), z = t / sqrt 2, branch-free.  1 + erf(z) = erfc(-z) = p(k) exp(-z^2) for z < 0 and 2 - p(k) exp(-z^2)
// for z >= 0, with k = 1 / (1 + 0.3275911 |z|) and p the degree-5 polynomial of Abramowitz & Stegun 7.1.26, whose error is at most
// 1.5e-7 ABSOLUTE on erf; with the hardware reciprocal and exp2 (1 ulp each) the error of gelu stays below 0.5 |t| * 3e-7, against
// the rounding to 16 bits that follows (2^-12 relative in fp16, 2^-9 in bf16).  The negative side takes erfc directly: no
// cancellation in 1 + erf.  (The device library's erff branches on |z|, both sides run inside a wave, and it costs 50 registers and
// a third of the time: profiles/EXPERIMENTS.md.)
__device__ __forceinline__ float sf_gelu(float t) {
  const float z = t * 0.70710678118654752440f;
  const float az = fabsf(z);
  const float k = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.f));
  float p = fmaf(k, 1.061405429f, -1.453152027f);
  p = fmaf(k, p, 1.421413741f);
  p = fmaf(k, p, -0.284496736f);
  p = fmaf(k, p, 0.254829592f);
  const float pe = (k * p) * __builtin_amdgcn_exp2f((az * az) * -1.44269504088896340736f);
  return (0.5f * t) * (z < 0.f ? pe : 2.f - pe);
}

template <bool BF16, int C>
__global__ __launch_bounds__(64, 2) void swin_ffn_kernel(SfArgs a) {
  constexpr int NT = SF_NT;
  constexpr int STR = C + 8, UPT = C / 8, KS = C / 32, CT = C / 16;
  __shared__ __attribute__((aligned(16))) unsigned short tile[SF_TOK * STR];

  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const long long t0 = (long long)blockIdx.x * SF_TOK;

  // ---- stage x ----
#pragma unroll
  for (int i = 0; i < UPT * NT / 4; ++i) {
    const int u = lane + 64 * i;
    const int tok = u / UPT, g = u - tok * UPT;
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (t0 + tok < a.T) v = *reinterpret_cast<const u32x4*>(a.x + (size_t)(t0 + tok) * C + 8 * g);
    *reinterpret_cast<u32x4*>(tile + tok * STR + 8 * g) = v;
  }
  __syncthreads();

  // ---- LayerNorm of token `lane`, in place ----
  if (lane < SF_TOK) {
    unsigned short* mine = tile + lane * STR;
    u32x4 row[UPT];
#pragma unroll
    for (int g = 0; g < UPT; ++g) row[g] = *reinterpret_cast<const u32x4*>(mine + 8 * g);
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < UPT; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += widen16<BF16>((unsigned short)(row[g][e >> 1] >> (16 * (e & 1))));
    const float mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int g = 0; g < UPT; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = widen16<BF16>((unsigned short)(row[g][e >> 1] >> (16 * (e & 1)))) - mean;
        sq = fmaf(d, d, sq);
      }
    const float rstd = 1.f / sqrtf(sq / (float)C + a.eps);
#pragma unroll
    for (int g = 0; g < UPT; ++g) {
      unsigned int h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = widen16<BF16>((unsigned short)(row[g][e >> 1] >> (16 * (e & 1)))) - mean;
        h[e] = round16<BF16>(fmaf(d * rstd, a.gamma[8 * g + e], a.beta[8 * g + e]));
      }
      *reinterpret_cast<u32x4*>(mine + 8 * g) = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    }
  }
  __syncthreads();

  // ---- the two products ----
  f32x4 acc[CT][NT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) acc[ct][tt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = a.hidden >> 5;
  const u32x4* w1p = a.w1 + lane;
  const u32x4* w2p = a.w2 + lane;
  const unsigned short* nb = tile + lr * STR + 8 * lg;   // the lane's B fragment of (token tile 0, k-step 0)
  u32x4 w1f[2][KS];
#pragma unroll
  for (int jt = 0; jt < 2; ++jt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) w1f[jt][ks] = w1p[(size_t)(jt * KS + ks) * 64];

  for (int s = 0; s < steps; ++s) {
    float4 bb[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) bb[jt] = *reinterpret_cast<const float4*>(a.b1 + 32 * s + 16 * jt + 4 * lg);

    f32x4 h[2][NT];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) h[jt][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // n is read from LDS again in every step: the empty asm keeps the compiler from hoisting the 16 KS registers of fragments out
    // of the loop (profiles/EXPERIMENTS.md)
    int noff = 0;                                           // (an offset, not the pointer: the reads stay LDS reads)
    asm volatile("" : "+v"(noff));
    const unsigned short* nbs = nb + noff;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        const u32x4 nf = *reinterpret_cast<const u32x4*>(nbs + 16 * tt * STR + 32 * ks);
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) h[jt][tt] = mfma16<BF16>(w1f[jt][ks], nf, h[jt][tt]);
      }

    // W2 of this step and W1 of the next are requested here and fly under the GELU (the last step asks for its own W1 again:
    // inside the array)
    u32x4 w2f[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) w2f[ct] = w2p[((size_t)s * CT + ct) * 64];
    const int sn = s + 1 < steps ? s + 1 : s;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) w1f[jt][ks] = w1p[((size_t)(2 * sn + jt) * KS + ks) * 64];

    u32x4 hf[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      unsigned int r[8];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        r[4 * jt + 0] = round16<BF16>(sf_gelu(h[jt][tt][0] + bb[jt].x));
        r[4 * jt + 1] = round16<BF16>(sf_gelu(h[jt][tt][1] + bb[jt].y));
        r[4 * jt + 2] = round16<BF16>(sf_gelu(h[jt][tt][2] + bb[jt].z));
        r[4 * jt + 3] = round16<BF16>(sf_gelu(h[jt][tt][3] + bb[jt].w));
      }
      hf[tt] = u32x4{r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16)};
    }

#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) acc[ct][tt] = mfma16<BF16>(w2f[ct], hf[tt], acc[ct][tt]);
  }

  // ---- residual and store ----
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const long long tok = t0 + 16 * tt + lr;
    if (tok >= a.T) continue;
    const unsigned short* xs = a.x + (size_t)tok * C + 4 * lg;
    unsigned short* dst = a.out + (size_t)tok * C + 4 * lg;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      float xr[4];
      widen4<BF16>(*reinterpret_cast<const u32x2*>(xs + 16 * ct), xr);
      const float4 b2 = *reinterpret_cast<const float4*>(a.b2 + 16 * ct + 4 * lg);
      const unsigned short r0 = round16<BF16>(xr[0] + (acc[ct][tt][0] + b2.x));
      const unsigned short r1 = round16<BF16>(xr[1] + (acc[ct][tt][1] + b2.y));
      const unsigned short r2 = round16<BF16>(xr[2] + (acc[ct][tt][2] + b2.z));
      const unsigned short r3 = round16<BF16>(xr[3] + (acc[ct][tt][3] + b2.w));
      *reinterpret_cast<u32x2*>(dst + 16 * ct) = pack4(r0, r1, r2, r3);
    }
  }
}

template <bool BF16, int C>
static void sf_launch(const SfArgs& a, hipStream_t stream) {
  const unsigned grid = (unsigned)((a.T + SF_TOK - 1) / SF_TOK);      // <= 2^29
  swin_ffn_kernel<BF16, C><<<dim3(grid), dim3(64), 0, stream>>>(a);
}

template <bool BF16>
static void sf_dispatch(const SfArgs& a, int channels, hipStream_t stream) {
  switch (channels) {
    case 32: sf_launch<BF16, 32>(a, stream); break;
    case 64: sf_launch<BF16, 64>(a, stream); break;
    case 96: sf_launch<BF16, 96>(a, stream); break;
    case 128: sf_launch<BF16, 128>(a, stream); break;
    case 160: sf_launch<BF16, 160>(a, stream); break;
    default: sf_launch<BF16, 192>(a, stream); break;
  }
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_swin_ffn_forward(const void* x, long long x_elems, const float* gamma, long long gamma_elems, const float* beta,
                            long long beta_elems, const void* packed1, long long packed1_elems, const float* b1, long long b1_elems,
                            const void* packed2, long long packed2_elems, const float* b2, long long b2_elems, int dtype,
                            long long tokens, int channels, int hidden, float eps, void* out, long long out_elems, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (channels < 32 || channels > SF_CMAX || channels % 32) {
    set_error("swin_ffn_forward: not supported (%d channels; the kernel is built for multiples of 32 from 32 to %d)", channels, SF_CMAX);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (hidden < 32 || hidden > SF_HMAX || hidden % 32) {
    set_error("swin_ffn_forward: not supported (%d hidden units; the kernel is built for multiples of 32 from 32 to %d)", hidden, SF_HMAX);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "swin_ffn_forward: dtype %d (0: fp16, 1: bf16)", dtype);
  BEVAMD_REQUIRE(eps > 0.f && eps - eps == 0.f, "swin_ffn_forward: eps is not a finite positive number");
  BEVAMD_REQUIRE(tokens >= 0 && tokens <= (1LL << 34), "swin_ffn_forward: %lld tokens (0 .. 2^34)", tokens);
  const long long want_x = tokens * channels, want_w = (long long)hidden * channels;
  BEVAMD_REQUIRE(x_elems == want_x, "swin_ffn_forward: x holds %lld elements, [%lld, %d] needs %lld", x_elems, tokens, channels, want_x);
  BEVAMD_REQUIRE(out_elems == want_x, "swin_ffn_forward: out holds %lld elements, [%lld, %d] needs %lld", out_elems, tokens, channels,
                 want_x);
  BEVAMD_REQUIRE(packed1_elems == want_w, "swin_ffn_forward: packed1 holds %lld elements, [%d, %d] needs %lld", packed1_elems, hidden,
                 channels, want_w);
  BEVAMD_REQUIRE(packed2_elems == want_w, "swin_ffn_forward: packed2 holds %lld elements, [%d, %d] needs %lld", packed2_elems, channels,
                 hidden, want_w);
  BEVAMD_REQUIRE(gamma_elems == channels && beta_elems == channels && b2_elems == channels,
                 "swin_ffn_forward: gamma, beta, b2 hold %lld, %lld, %lld floats, each needs %d", gamma_elems, beta_elems, b2_elems, channels);
  BEVAMD_REQUIRE(b1_elems == hidden, "swin_ffn_forward: b1 holds %lld floats, needs %d", b1_elems, hidden);
  BEVAMD_REQUIRE(gamma != nullptr && beta != nullptr && b1 != nullptr && b2 != nullptr && packed1 != nullptr && packed2 != nullptr,
                 "swin_ffn_forward: gamma, beta, b1, b2, packed1 or packed2 is null");
  BEVAMD_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)packed1 | (uintptr_t)packed2) & 15) == 0,
                 "swin_ffn_forward: gamma, beta, b1, b2, packed1 or packed2 is not 16-byte aligned");
  if (tokens == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(x != nullptr && out != nullptr, "swin_ffn_forward: x or out is null");
  BEVAMD_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "swin_ffn_forward: x or out is not 16-byte aligned");
  BEVAMD_REQUIRE(!ranges_overlap(out, 2 * want_x, x, 2 * want_x), "swin_ffn_forward: out overlaps x");
  BEVAMD_REQUIRE(!ranges_overlap(out, 2 * want_x, packed1, 2 * want_w) && !ranges_overlap(out, 2 * want_x, packed2, 2 * want_w),
                 "swin_ffn_forward: out overlaps packed1 or packed2");
  BEVAMD_REQUIRE(!ranges_overlap(out, 2 * want_x, gamma, 4LL * channels) && !ranges_overlap(out, 2 * want_x, beta, 4LL * channels) &&
                     !ranges_overlap(out, 2 * want_x, b1, 4LL * hidden) && !ranges_overlap(out, 2 * want_x, b2, 4LL * channels),
                 "swin_ffn_forward: out overlaps gamma, beta, b1 or b2");

  SfArgs a;
  a.x = (const unsigned short*)x;
  a.gamma = gamma;
  a.beta = beta;
  a.b1 = b1;
  a.b2 = b2;
  a.w1 = (const u32x4*)packed1;
  a.w2 = (const u32x4*)packed2;
  a.out = (unsigned short*)out;
  a.T = tokens;
  a.hidden = hidden;
  a.eps = eps;
  if (dtype == 1)
    sf_dispatch<true>(a, channels, stream);
  else
    sf_dispatch<false>(a, channels, stream);
  BEVAMD_LAUNCH_CHECK("swin_ffn");
  return BEVAMD_OK;
}

}  // extern "C"
