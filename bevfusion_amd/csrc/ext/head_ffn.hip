// The learned ends of TransFusionHead.forward_single that are not the decoder layer, gfx950.
//
// Replaces (reference, mmdet3d/models/heads/bbox/transfusion.py and mmdet3d/models/utils/transformer.py):
//   transfusion.py:283-288   one_hot -> permute -> float -> Conv1d(num_classes, C, 1) -> query_feat += ...      (5 launches)
//   transfusion.py:311-312   FFN.forward (transformer.py:496-575): per head Conv1d -> BatchNorm1d -> ReLU -> Conv1d, then
//                            center + query_pos.permute(0, 2, 1), and the torch.cat over the layers             (~25 launches)
//
// Native formulation:
//   * bevamd_head_class_encoding: a 1x1 convolution over a one-hot vector is a column lookup; one thread per element adds
//     weight[c, label] + bias[c] in place.  The reference's convolution adds exact zeros to that one product (1.0f * w), so the
//     result is bit-equal to its fp32 arithmetic.  The unit is compiled with fp contract(off).
//   * bevamd_head_ffn_forward: ONE launch for all heads of a decoder layer in eval mode.  A workgroup owns (sample, tile of
//     HF_TP query columns, head): it stages the [Cin, HF_TP] input tile in LDS, computes the head's [head_conv, HF_TP] hidden tile
//     as a register-tiled fp32 FMA GEMM (4 hidden rows x 4 columns per thread, the first conv's weight read 16 bytes at a time
//     along Cin), applies the folded BatchNorm and the ReLU into LDS, and computes the [c_h, HF_TP] output tile from there with
//     the bias and, for the center head, query_pos.  The hidden activations never reach memory.  Every output element is the sum
//     of one thread in ascending channel order: no atomics, equal calls give equal bits.
//     At B = 8, P = 200 the whole problem is 1 600 columns: the grid comes from (tile, head, sample) = 13 x 6 x 8 workgroups of two
//     waves; a wider tile would leave most of the 256 compute units without work.
#include "common.h"

#pragma clang fp contract(off)

namespace bevamd {

constexpr int HF_TP = 16;            // query columns per workgroup
constexpr int HF_THREADS = 128;      // one thread per (4 hidden rows, 4 columns): head_conv <= 128
constexpr int HF_MAX_CIN = 256;
constexpr int HF_MAX_HC = 128;
constexpr int HF_MAX_C = 32;
constexpr int HF_MAX_HEADS = 8;

struct HfHeads {
  int c[HF_MAX_HEADS];                 // output channels
  const float* w1[HF_MAX_HEADS];       // [head_conv, Cin]
  const float* scale[HF_MAX_HEADS];    // folded BatchNorm [head_conv]
  const float* shift[HF_MAX_HEADS];
  const float* w2[HF_MAX_HEADS];       // [c, head_conv]
  const float* bias[HF_MAX_HEADS];     // [c]
  float* out[HF_MAX_HEADS];            // [B, c, out_stride]
};

__global__ __launch_bounds__(256) void head_class_encoding_kernel(float* __restrict__ query_feat, const long long* __restrict__ labels,
                                                                  const float* __restrict__ weight, const float* __restrict__ bias,
                                                                  long long total, int C, int K, int num_classes) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int k = (int)(e % K);
    const long long bc = e / K;
    const int c = (int)(bc % C);
    const long long b = bc / C;
    const long long l = labels[b * K + k];
    if (l < 0 || l >= num_classes) continue;   // one_hot raises there; nothing is added and nothing outside weight is read
    const float enc = weight[(size_t)c * num_classes + l] + bias[c];
    query_feat[e] = query_feat[e] + enc;
  }
}

__global__ __launch_bounds__(HF_THREADS) void head_ffn_kernel(const float* __restrict__ x, const float* __restrict__ query_pos, int Cin,
                                                              int HC, int P, int out_stride, int col_offset, int center_head,
                                                              HfHeads heads) {
  __shared__ __attribute__((aligned(16))) float xs[HF_MAX_CIN * HF_TP];   // xs[k][p]: the input tile
  __shared__ __attribute__((aligned(16))) float hs[HF_MAX_HC * HF_TP];    // hs[j][p]: the hidden tile after BatchNorm and ReLU

  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * HF_TP;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int np = min(HF_TP, P - p0);   // >= 1: the grid has cdiv(P, HF_TP) tiles

  // columns past P are zero: they are computed and never stored
  const float* xb = x + (size_t)b * Cin * P + p0;
  for (int idx = tid; idx < Cin * HF_TP; idx += HF_THREADS) {
    const int k = idx / HF_TP, p = idx - k * HF_TP;
    xs[idx] = p < np ? xb[(size_t)k * P + p] : 0.f;
  }
  __syncthreads();

  if (tid < HC) {   // HC is a multiple of 16: HC / 4 row groups x 4 column groups
    const int rq = tid >> 2, cq = tid & 3;
    const float* w = heads.w1[h] + (size_t)(rq * 4) * Cin;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k = 0; k < Cin; k += 4) {
      float wr[4][4], xv[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(w + (size_t)i * Cin + k);
        wr[i][0] = t.x; wr[i][1] = t.y; wr[i][2] = t.z; wr[i][3] = t.w;
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float4 t = *reinterpret_cast<const float4*>(xs + (k + kk) * HF_TP + cq * 4);
        xv[kk][0] = t.x; xv[kk][1] = t.y; xv[kk][2] = t.z; xv[kk][3] = t.w;
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(wr[i][kk], xv[kk][j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rq * 4 + i;
      const float s = heads.scale[h][row], t = heads.shift[h][row];
      float4 o;
      o.x = fmaxf(fmaf(acc[i][0], s, t), 0.f);
      o.y = fmaxf(fmaf(acc[i][1], s, t), 0.f);
      o.z = fmaxf(fmaf(acc[i][2], s, t), 0.f);
      o.w = fmaxf(fmaf(acc[i][3], s, t), 0.f);
      *reinterpret_cast<float4*>(hs + row * HF_TP + cq * 4) = o;
    }
  }
  __syncthreads();

  const int c = heads.c[h];
  const float* w2 = heads.w2[h];
  float* out = heads.out[h] + (size_t)b * c * out_stride + col_offset + p0;
  for (int idx = tid; idx < c * HF_TP; idx += HF_THREADS) {
    const int cc = idx / HF_TP, p = idx - cc * HF_TP;
    float acc = 0.f;
    for (int j = 0; j < HC; j += 4) {
      const float4 wv = *reinterpret_cast<const float4*>(w2 + (size_t)cc * HC + j);
      acc = fmaf(wv.x, hs[(j + 0) * HF_TP + p], acc);
      acc = fmaf(wv.y, hs[(j + 1) * HF_TP + p], acc);
      acc = fmaf(wv.z, hs[(j + 2) * HF_TP + p], acc);
      acc = fmaf(wv.w, hs[(j + 3) * HF_TP + p], acc);
    }
    if (p >= np) continue;
    float v = acc + heads.bias[h][cc];
    if (query_pos != nullptr && h == center_head) v = v + query_pos[((size_t)b * P + p0 + p) * 2 + cc];
    out[(size_t)cc * out_stride + p] = v;
  }
}

static bool hf_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_head_class_encoding(float* query_feat, const long long* labels, const float* weight, const float* bias, int batch,
                               int channels, int num_queries, int num_classes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 0 && channels >= 1 && num_queries >= 1 && num_classes >= 1,
                 "head_class_encoding: bad sizes (B %d, C %d, K %d, classes %d)", batch, channels, num_queries, num_classes);
  BEVAMD_REQUIRE(query_feat && labels && weight && bias, "head_class_encoding: null buffer");
  if (batch == 0) return BEVAMD_OK;
  const long long total = (long long)batch * channels * num_queries;
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  head_class_encoding_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(query_feat, labels, weight, bias, total, channels,
                                                                             num_queries, num_classes);
  BEVAMD_LAUNCH_CHECK("head_class_encoding");
  return BEVAMD_OK;
}

int bevamd_head_ffn_forward(const float* x, int batch, int in_channels, int num_queries, int head_conv, int num_heads,
                            const int* head_channels, const void* const* w1, const void* const* scales, const void* const* shifts,
                            const void* const* w2, const void* const* biases, const float* query_pos, int center_head,
                            void* const* outs, int out_stride, int col_offset, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(head_channels && w1 && scales && shifts && w2 && biases && outs, "head_ffn_forward: null host array");
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "head_ffn_forward: batch %d (0 .. 65535)", batch);
  if (num_heads < 1 || num_heads > HF_MAX_HEADS || in_channels < 4 || in_channels > HF_MAX_CIN || (in_channels & 3) || head_conv < 16 ||
      head_conv > HF_MAX_HC || (head_conv & 15) || num_queries < 1 || col_offset < 0 ||
      (long long)col_offset + num_queries > (long long)out_stride) {
    set_error("head_ffn_forward: not supported (%d heads of 1 .. %d; Cin %d a multiple of 4 up to %d; head_conv %d a multiple of 16 up "
              "to %d; P %d >= 1 in columns [%d, %d) of %d)", num_heads, HF_MAX_HEADS, in_channels, HF_MAX_CIN, head_conv, HF_MAX_HC,
              num_queries, col_offset, col_offset + num_queries, out_stride);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  HfHeads heads;
  for (int h = 0; h < HF_MAX_HEADS; ++h) {
    heads.c[h] = 0;
    heads.w1[h] = heads.scale[h] = heads.shift[h] = heads.w2[h] = heads.bias[h] = nullptr;
    heads.out[h] = nullptr;
  }
  for (int h = 0; h < num_heads; ++h) {
    const int c = head_channels[h];
    if (c < 1 || c > HF_MAX_C) {
      set_error("head_ffn_forward: not supported (head %d has %d channels, 1 .. %d)", h, c, HF_MAX_C);
      return BEVAMD_ERR_UNSUPPORTED;
    }
    BEVAMD_REQUIRE(w1[h] && scales[h] && shifts[h] && w2[h] && biases[h] && outs[h], "head_ffn_forward: head %d has a null pointer", h);
    BEVAMD_REQUIRE(hf_aligned16(w1[h]) && hf_aligned16(w2[h]), "head_ffn_forward: the weights of head %d are not 16-byte aligned", h);
    heads.c[h] = c;
    heads.w1[h] = (const float*)w1[h];
    heads.scale[h] = (const float*)scales[h];
    heads.shift[h] = (const float*)shifts[h];
    heads.w2[h] = (const float*)w2[h];
    heads.bias[h] = (const float*)biases[h];
    heads.out[h] = (float*)outs[h];
  }
  if (query_pos == nullptr) center_head = -1;
  if (center_head >= 0)
    BEVAMD_REQUIRE(center_head < num_heads && head_channels[center_head] == 2,
                   "head_ffn_forward: center_head %d must name a head of 2 channels (query_pos is [B, P, 2])", center_head);
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(x != nullptr, "head_ffn_forward: x is null");
  const dim3 grid(cdiv(num_queries, HF_TP), num_heads, batch);
  head_ffn_kernel<<<grid, dim3(HF_THREADS), 0, stream>>>(x, center_head >= 0 ? query_pos : nullptr, in_channels, head_conv, num_queries,
                                                         out_stride, col_offset, center_head, heads);
  BEVAMD_LAUNCH_CHECK("head_ffn");
  return BEVAMD_OK;
}

}  // extern "C"
