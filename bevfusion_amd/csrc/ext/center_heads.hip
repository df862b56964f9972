// The task heads of CenterHead.forward_single in eval mode, gfx950.
//
// Replaces (reference, mmdet3d/models/heads/bbox/centerpoint.py):
//   centerpoint.py:121-125   SeparateHead.forward: per head Conv2d(64 -> 64, k x k, no bias) -> BatchNorm2d -> ReLU -> Conv2d(64 -> c, k x k)
//   centerpoint.py:351-352   CenterHead.forward_single: that for every task (nuScenes: 6 tasks x 6 heads x 4 layers = 144 launches)
//
// Native formulation: ONE launch.  A workgroup of four waves (256 threads) owns (spatial tile, task, sample) and loops over the task's heads:
//   1. the input tile of the shared map with a halo of 2 * (k / 2) cells is staged in LDS once for all heads, zero outside the map;
//   2. the hidden tile (8 x 16 = 128 cells, halo k / 2) is an implicit GEMM D[channel][cell] = W[channel][(tap, ci)] * X[(tap, ci)][cell]
//      with K = 64 * k * k on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain): wave w owns the channel tile w & 1 and the
//      cell tiles 2 * (w >> 1) and 2 * (w >> 1) + 1, so one weight fragment feeds two cell tiles; the k-steps go to four
//      interleaved accumulators (step mod 4) that are added pairwise at the end;
//   3. the weights are packed on the host in the lane order of the A fragment (four k-steps per lane = one 16-byte load) and
//      stream from global / L2; the B fragment is one LDS dword per lane and step;
//   4. scale, shift and ReLU go into the hidden tile in LDS; a hidden cell OUTSIDE the map is written as zero: the second
//      convolution pads the hidden map with zeros and relu(shift) is not zero;
//   5. the c-channel output convolution is, per output element, four fp32 fmaf chains (channel mod 4) in (tap, channel) order from
//      the hidden tile, added pairwise, plus the bias, stored along W.
// The hidden activations never reach memory.  Every hidden value is the sum of one lane's four accumulators and every output
// element the sum of one thread, both in a fixed order: no atomics, equal calls give equal bits, and a sample's result does not
// depend on the batch around it.
#include "common.h"

#pragma clang fp contract(off)

namespace bevamd {

constexpr int CH_C = 64;                       // channels of the shared map and of the hidden map
#ifndef BEVAMD_CH_TILE_ROWS
#define BEVAMD_CH_TILE_ROWS 8                  // 16: the 14 x 14 output tile of profiles/EXPERIMENTS.md (one workgroup of 8 waves per CU)
#endif
constexpr int CH_HT_H = BEVAMD_CH_TILE_ROWS, CH_HT_W = 16;   // hidden tile: 128 cells = 4 MFMA column tiles of 32
constexpr int CH_CELLS = CH_HT_H * CH_HT_W;
constexpr int CH_THREADS = 32 * CH_HT_H;       // one wave per (channel tile, pair of cell tiles)
static_assert(CH_HT_H == 8 || CH_HT_H == 16, "the hidden tile has 8 or 16 rows");
constexpr int CH_MAX_TASKS = 8;
constexpr int CH_MAX_TASK_HEADS = 8;
constexpr int CH_MAX_HEADS = CH_MAX_TASKS * CH_MAX_TASK_HEADS;
constexpr int CH_MAX_C = 16;

struct ChTable {                               // by value: about 1 KB of the 4 KB kernel-argument segment
  int task_begin[CH_MAX_TASKS + 1];            // task t owns the heads [task_begin[t], task_begin[t + 1])
  int c[CH_MAX_HEADS];                         // output channels
  int cprefix[CH_MAX_HEADS];                   // output channels of the heads before it: the head's block starts at cprefix * B * H * W
  long long off[CH_MAX_HEADS];                 // first float of the head's block in `packed`
};

typedef float ch_f32x16 __attribute__((ext_vector_type(16)));

// floats of one head's block: w1 in fragment order, scale, shift, w2 as [c][tap][64], bias padded to 4
static inline long long ch_block_floats(int k2, int c) {
  return (long long)CH_C * CH_C * k2 + 2 * CH_C + (long long)c * k2 * CH_C + ((c + 3) & ~3);
}

template <int KS>
__global__ __launch_bounds__(CH_THREADS, 16 / CH_HT_H) void center_heads_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                                  float* __restrict__ out, int B, int H, int W, int tiles_x, ChTable tab) {
  constexpr int P = KS / 2, K2 = KS * KS;
  constexpr int OH = CH_HT_H - 2 * P, OW = CH_HT_W - 2 * P;   // output tile
  constexpr int XH = CH_HT_H + 2 * P, XW = CH_HT_W + 2 * P;   // input tile
  constexpr int XP = XH * XW;
  __shared__ __attribute__((aligned(16))) float xs[CH_C * XP];        // xs[ci][iy][ix]
  __shared__ __attribute__((aligned(16))) float hs[CH_C * CH_CELLS];  // hs[channel][hidden cell] after BatchNorm and ReLU

  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int t = blockIdx.y, b = blockIdx.z;
  const int oy0 = ty * OH, ox0 = tx * OW;
  const size_t hw = (size_t)H * W;

  const float* xb = x + (size_t)b * CH_C * hw;
  for (int idx = tid; idx < CH_C * XP; idx += CH_THREADS) {
    const int ci = idx / XP, rem = idx - ci * XP;
    const int iy = rem / XW, ix = rem - iy * XW;
    const int gy = oy0 - 2 * P + iy, gx = ox0 - 2 * P + ix;
    xs[idx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[(size_t)ci * hw + (size_t)gy * W + gx] : 0.f;
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int m = wave & 1, ct0 = (wave >> 1) * 2;
  const int half = lane >> 5, n = lane & 31;
  // B fragment: lane holds X[k = 2 s + half][cell n] of the cell tile; cell = (row 2 ct + (n >> 4), column n & 15) of the hidden tile
  const int boff0 = half * XP + (2 * ct0 + (n >> 4)) * XW + (n & 15);
  const int boff1 = boff0 + 2 * XW;

  for (int h = tab.task_begin[t]; h < tab.task_begin[t + 1]; ++h) {
    const float* blk = packed + tab.off[h];
    const float4* wa = reinterpret_cast<const float4*>(blk) + (size_t)m * (K2 * 8 * 64) + lane;
    // four interleaved chains per cell tile (k-step mod 4), combined pairwise below: a quarter of the length of one chain, and
    // about half its rounding error, at the same MFMA count
    ch_f32x16 acc0[4], acc1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc0[q][r] = 0.f; acc1[q][r] = 0.f; }
#pragma unroll 1
    for (int tap = 0; tap < K2; ++tap) {
      const int toff = (tap / KS) * XW + (tap % KS);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float4 a4 = wa[(tap * 8 + g) * 64];
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ci0 = g * 8 + q * 2;
          const float b0 = xs[ci0 * XP + boff0 + toff];
          const float b1 = xs[ci0 * XP + boff1 + toff];
          acc0[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], b0, acc0[q], 0, 0, 0);
          acc1[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], b1, acc1[q], 0, 0, 0);
        }
      }
    }

    const float* scale = blk + (size_t)CH_C * CH_C * K2;
    const float* shift = scale + CH_C;
    // D fragment: column (cell) on the lane, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 half
    const int r0 = 2 * ct0 + (n >> 4), cx = n & 15;
    const int gx = ox0 - P + cx;
    const bool in_x = gx >= 0 && gx < W;
    const int gy0 = oy0 - P + r0, gy1 = gy0 + 2;
    const bool in0 = in_x && gy0 >= 0 && gy0 < H, in1 = in_x && gy1 >= 0 && gy1 < H;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ch = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const float s = scale[ch], sh = shift[ch];
      const float d0 = (acc0[0][r] + acc0[1][r]) + (acc0[2][r] + acc0[3][r]);
      const float d1 = (acc1[0][r] + acc1[1][r]) + (acc1[2][r] + acc1[3][r]);
      hs[ch * CH_CELLS + ct0 * 32 + n] = in0 ? fmaxf(fmaf(d0, s, sh), 0.f) : 0.f;
      hs[ch * CH_CELLS + ct0 * 32 + 32 + n] = in1 ? fmaxf(fmaf(d1, s, sh), 0.f) : 0.f;
    }
    __syncthreads();

    const int c = tab.c[h];
    const float* w2 = shift + CH_C;                  // [c][tap][64]
    const float* bias = w2 + (size_t)c * K2 * CH_C;
    float* ob = out + ((size_t)tab.cprefix[h] * B + (size_t)b * c) * hw;
    for (int idx = tid; idx < c * OH * OW; idx += CH_THREADS) {
      const int cc = idx / (OH * OW), cell = idx - cc * (OH * OW);
      const int oy = cell / OW, ox = cell - oy * OW;
      const int gy = oy0 + oy, gxo = ox0 + ox;
      if (gy >= H || gxo >= W) continue;
      const float* w = w2 + (size_t)cc * K2 * CH_C;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four chains (channel mod 4), combined pairwise
      for (int tap = 0; tap < K2; ++tap) {
        const float* hb = hs + (oy + tap / KS) * CH_HT_W + ox + tap % KS;
#pragma unroll 4
        for (int j = 0; j < CH_C; j += 4) {
          const float4 wv = *reinterpret_cast<const float4*>(w + tap * CH_C + j);
          a0 = fmaf(wv.x, hb[(j + 0) * CH_CELLS], a0);
          a1 = fmaf(wv.y, hb[(j + 1) * CH_CELLS], a1);
          a2 = fmaf(wv.z, hb[(j + 2) * CH_CELLS], a2);
          a3 = fmaf(wv.w, hb[(j + 3) * CH_CELLS], a3);
        }
      }
      ob[(size_t)cc * hw + (size_t)gy * W + gxo] = ((a0 + a1) + (a2 + a3)) + bias[cc];
    }
    __syncthreads();   // the next head overwrites the hidden tile
  }
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_center_heads_forward(const float* x, int batch, int channels, int head_conv, int height, int width, int final_kernel,
                                int num_tasks, const int* heads_per_task, const int* head_channels, const float* packed,
                                long long packed_floats, float* out, long long out_floats, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(heads_per_task && head_channels, "center_heads_forward: null host array");
  BEVAMD_REQUIRE(batch >= 0 && batch <= 65535, "center_heads_forward: batch %d (0 .. 65535)", batch);
  BEVAMD_REQUIRE(height >= 1 && width >= 1, "center_heads_forward: bad sizes (H %d, W %d)", height, width);
  if (channels != CH_C || head_conv != CH_C || (final_kernel != 1 && final_kernel != 3) || num_tasks < 1 || num_tasks > CH_MAX_TASKS) {
    set_error("center_heads_forward: not supported (channels %d and head_conv %d must be %d; final_kernel %d of 1 or 3; %d tasks of 1 .. %d)",
              channels, head_conv, CH_C, final_kernel, num_tasks, CH_MAX_TASKS);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  const int k2 = final_kernel * final_kernel;
  ChTable tab;
  for (int h = 0; h < CH_MAX_HEADS; ++h) { tab.c[h] = 0; tab.cprefix[h] = 0; tab.off[h] = 0; }
  int heads = 0, sumc = 0;
  long long floats = 0;
  for (int t = 0; t < num_tasks; ++t) {
    const int nh = heads_per_task[t];
    if (nh < 1 || nh > CH_MAX_TASK_HEADS) {
      set_error("center_heads_forward: not supported (task %d has %d heads, 1 .. %d)", t, nh, CH_MAX_TASK_HEADS);
      return BEVAMD_ERR_UNSUPPORTED;
    }
    tab.task_begin[t] = heads;
    for (int i = 0; i < nh; ++i, ++heads) {
      const int c = head_channels[heads];
      if (c < 1 || c > CH_MAX_C) {
        set_error("center_heads_forward: not supported (head %d of task %d has %d channels, 1 .. %d)", i, t, c, CH_MAX_C);
        return BEVAMD_ERR_UNSUPPORTED;
      }
      tab.c[heads] = c;
      tab.cprefix[heads] = sumc;
      tab.off[heads] = floats;
      sumc += c;
      floats += ch_block_floats(k2, c);
    }
  }
  for (int t = num_tasks; t <= CH_MAX_TASKS; ++t) tab.task_begin[t] = heads;
  const int OH = CH_HT_H - 2 * (final_kernel / 2), OW = CH_HT_W - 2 * (final_kernel / 2);
  const long long tiles_x = cdiv(width, OW), tiles = tiles_x * cdiv(height, OH);
  BEVAMD_REQUIRE(tiles <= 0x7fffffffLL, "center_heads_forward: a %d x %d map has too many tiles", height, width);
  BEVAMD_REQUIRE(packed_floats == floats, "center_heads_forward: packed holds %lld floats, these heads need %lld", packed_floats, floats);
  const long long want_out = (long long)batch * sumc * height * width;
  BEVAMD_REQUIRE(out_floats == want_out, "center_heads_forward: out holds %lld floats, [%d, %d, %d, %d] needs %lld", out_floats, batch,
                 sumc, height, width, want_out);
  BEVAMD_REQUIRE(packed != nullptr && ((uintptr_t)packed & 15) == 0, "center_heads_forward: packed is null or not 16-byte aligned");
  if (batch == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(x != nullptr && out != nullptr, "center_heads_forward: x or out is null");
  const dim3 grid((unsigned)tiles, num_tasks, batch);
  if (final_kernel == 3)
    center_heads_kernel<3><<<grid, dim3(CH_THREADS), 0, stream>>>(x, packed, out, batch, height, width, (int)tiles_x, tab);
  else
    center_heads_kernel<1><<<grid, dim3(CH_THREADS), 0, stream>>>(x, packed, out, batch, height, width, (int)tiles_x, tab);
  BEVAMD_LAUNCH_CHECK("center_heads");
  return BEVAMD_OK;
}

}  // extern "C"
