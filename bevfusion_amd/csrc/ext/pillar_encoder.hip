// Pillar / radar feature nets and the pseudo-image scatter (PointPillars family), gfx950.
//
// Replaces (reference, mmdet3d/models/backbones/pillar_encoder.py and radar_encoder.py):
//   PillarFeatureNet.forward / RadarFeatureNet.forward   decorations by slicing + cat, a [M, P, C] tensor per layer
//   PFNLayer / RFNLayer                                  Linear (no bias) -> BatchNorm1d -> ReLU -> max over the P rows
//   PointPillarsScatter.forward                          a Python loop over the batch with a boolean mask and an index_put
//
// Native formulation:
//   * bevamd_pillar_decorate: one thread per element of the decorated [M, P, F_out] tensor (the training path feeds it to the
//     module's own torch layers).  The unit is compiled with fp contract(off): no FMA
//     contraction, so every column except f_cluster (a sum whose order is free) is bit-equal to the reference's fp32 result.
//   * bevamd_pillar_stack_forward: the eval-mode network.  A workgroup owns PS_CHUNK consecutive pillars and packs their REAL
//     rows, plus ONE all-zero row per pillar that has padding (every padded row of a pillar is identical in every layer, and it
//     takes part in the max), into tiles of at most PS_ROWS rows.  A tile lives in LDS as act[k][row]; every layer is a
//     register-tiled fp32 FMA GEMM (8 rows x 4 columns per thread) against the layer's weights, staged into LDS in chunks of
//     PS_KC input channels, followed by the folded BatchNorm + ReLU, written back IN PLACE, and the layer's combine rule.
//     Only [M, C_last] goes to global memory.
//   * bevamd_pillar_scatter_forward / _backward: atomicMax of the row id into an int32 winner plane (the highest row wins a
//     duplicated cell: what the reference's sequential index_put leaves), then one coalesced pass over the whole canvas that
//     writes the winner's value or zero.  Integer atomics only: deterministic.
#include "common.h"

#include <float.h>
#include <math.h>

// No FMA contraction anywhere in this unit: the decorations must round like the reference's separate fp32 multiply and add.
// The __fmul_rn / __fadd_rn intrinsics do not give that: they are inline `x * y` / `x + y` of a header parsed under the
// default contraction mode, and a multiply feeding an add still fuses after inlining.  The operators below are written
// under the pragma and carry no contraction flag.  The GEMM asks for its FMAs explicitly (fmaf).
#pragma clang fp contract(off)

namespace bevamd {

constexpr int PE_MAX_P = 32;        // rows per pillar
constexpr int PE_MAX_WIDTH = 128;   // widest layer
constexpr int PE_MAX_IN = 64;       // raw point width
constexpr int PE_MAX_LAYERS = 4;
enum { PE_PILLAR = 0, PE_RADAR = 1 };

struct PeGeom {
  float vx, vy, xo, yo;   // voxel size and the centre of cell 0, rounded once from the host's doubles
  float lo[3], span[3];   // radar: xyz -> (v - lo) / span, span = fp32(hi - lo)
};

__device__ __forceinline__ float pe_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float pe_add(float a, float b) { return a + b; }
__device__ __forceinline__ float pe_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float pe_div(float a, float b) { return a / b; }   // correctly rounded: no fast-math in this build

// sum_over_P(xyz[d]) / num_points: all P rows in ascending order (padded rows are part of the reference's sum)
__device__ __forceinline__ float pe_mean(const float* __restrict__ vox, int P, int F, int d, int num) {
  float s = 0.f;
  for (int p = 0; p < P; ++p) s = pe_add(s, vox[p * F + d]);
  return pe_div(s, (float)num);
}

__device__ __forceinline__ float pe_center(float v, int c, float size, float off) {
  return pe_sub(v, pe_add(pe_mul((float)c, size), off));
}

// element f of a decorated row, before the padding mask; mean_d: the pillar's mean of the column f_cluster column f refers to
__device__ __forceinline__ float pe_value(const float* __restrict__ row, int F, int f, int mode, const PeGeom& g, int cx, int cy,
                                          float mean_d) {
  if (mode == PE_RADAR) {
    if (f < 3) return pe_div(pe_sub(row[f], g.lo[f]), g.span[f]);
    if (f < F) return row[f];
    return f == F ? pe_center(row[0], cx, g.vx, g.xo) : pe_center(row[1], cy, g.vy, g.yo);
  }
  if (f < F) return row[f];
  if (f < F + 3) return pe_sub(row[f - F], mean_d);
  if (f == F + 3) return pe_center(row[0], cx, g.vx, g.xo);
  if (f == F + 4) return pe_center(row[1], cy, g.vy, g.yo);
  const float x = row[0], y = row[1], z = row[2];
  return __fsqrt_rn(pe_add(pe_add(pe_mul(x, x), pe_mul(y, y)), pe_mul(z, z)));
}

__device__ __forceinline__ float pe_nan_to_num(float v) {
  if (isnan(v)) return 0.f;
  if (isinf(v)) return copysignf(FLT_MAX, v);
  return v;
}

__global__ __launch_bounds__(256) void pillar_decorate_kernel(const float* __restrict__ vox, const int* __restrict__ num,
                                                              const int* __restrict__ coors, long long total, int P, int F, int Fo,
                                                              int mode, PeGeom g, float* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int f = (int)(e % Fo);
    const long long mp = e / Fo;
    const int p = (int)(mp % P);
    const long long m = mp / P;
    const float* pil = vox + (size_t)m * P * F;
    const int n = num[m];
    float mean_d = 0.f;
    if (mode == PE_PILLAR && f >= F && f < F + 3) mean_d = pe_mean(pil, P, F, f - F, n);
    float v = pe_value(pil + (size_t)p * F, F, f, mode, g, coors[m * 4 + 1], coors[m * 4 + 2], mean_d);
    v = pe_mul(v, p < n ? 1.f : 0.f);   // features *= mask
    if (mode == PE_RADAR) v = pe_nan_to_num(v);
    out[e] = v;
  }
}

// ---- fused eval-mode stack ----------------------------------------------------------------------------------------------
constexpr int PS_THREADS = 256;
constexpr int PS_CHUNK = 16;    // pillars per workgroup
constexpr int PS_ROWS = 64;     // rows per tile (>= PE_MAX_P: one pillar always fits)
constexpr int PS_RP = 68;       // row pitch of act[k][.]: 16-byte aligned rows, shifted by 4 banks per input channel
constexpr int PS_KC = 64;       // input channels of a staged weight chunk

struct PsNet {
  int n;
  int K[PE_MAX_LAYERS];     // input width
  int C[PE_MAX_LAYERS];     // units (Linear out_features)
  int cat[PE_MAX_LAYERS];   // append the per-pillar max (PFNLayer that is not the last)
  const float* w[PE_MAX_LAYERS];       // [K, C]: the Linear weight transposed
  const float* scale[PE_MAX_LAYERS];   // folded BatchNorm
  const float* shift[PE_MAX_LAYERS];
};

__global__ __launch_bounds__(PS_THREADS, 2) void pillar_stack_kernel(const float* __restrict__ vox, const int* __restrict__ num,
                                                                     const int* __restrict__ coors, int M, int P, int F, int Fo,
                                                                     int mode, PeGeom g, PsNet net, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float act[PE_MAX_WIDTH * PS_RP];   // act[k][row]: one tile, updated in place
  __shared__ __attribute__((aligned(16))) float wl[PS_KC * PE_MAX_WIDTH];    // wl[k][c]: one chunk of one layer's weights
  __shared__ float s_mean[PS_CHUNK * 3];
  __shared__ int s_n[PS_CHUNK];          // real rows of every pillar of the chunk, clamped to [0, P]
  __shared__ int s_start[PS_CHUNK + 1];  // first tile row of every pillar of the tile
  __shared__ short s_rowp[PS_ROWS];      // tile row -> pillar of the chunk
  __shared__ short s_rowpt[PS_ROWS];     // tile row -> point of the pillar, -1: the pillar's padded row

  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * PS_CHUNK;
  const int cnt = min(PS_CHUNK, M - m0);
  if (tid < cnt) s_n[tid] = min(max(num[m0 + tid], 0), P);
  if (mode == PE_PILLAR && tid < cnt * 3) {
    const int p = tid / 3;
    s_mean[tid] = pe_mean(vox + (size_t)(m0 + p) * P * F, P, F, tid - p * 3, num[m0 + p]);
  }
  __syncthreads();

  int p0 = 0;
  while (p0 < cnt) {
    // the tile: pillars [p0, p1), as many as fit PS_ROWS rows (every thread walks the same few counts)
    int rows = 0, p1 = p0;
    while (p1 < cnt) {
      const int n = s_n[p1];
      const int r = n + (n < P ? 1 : 0);
      if (rows + r > PS_ROWS) break;
      rows += r;
      ++p1;
    }
    const int np = p1 - p0;
    if (tid < np) {
      int start = 0;
      for (int q = 0; q < tid; ++q) start += s_n[p0 + q] + (s_n[p0 + q] < P ? 1 : 0);
      const int n = s_n[p0 + tid];
      s_start[tid] = start;
      for (int i = 0; i < n; ++i) { s_rowp[start + i] = (short)(p0 + tid); s_rowpt[start + i] = (short)i; }
      if (n < P) { s_rowp[start + n] = (short)(p0 + tid); s_rowpt[start + n] = -1; }
      if (tid == np - 1) s_start[np] = rows;
    }
    __syncthreads();

    // layer 0 input: the decorated rows; the padded row and the rows that fill the last group of 8 are zero
    const int rows8 = (rows + 7) & ~7;
    for (int idx = tid; idx < rows8 * Fo; idx += PS_THREADS) {
      const int r = idx / Fo, f = idx - r * Fo;
      float v = 0.f;
      if (r < rows && s_rowpt[r] >= 0) {
        const int p = s_rowp[r];
        const size_t m = (size_t)(m0 + p);
        const float mean_d = (mode == PE_PILLAR && f >= F && f < F + 3) ? s_mean[p * 3 + f - F] : 0.f;
        v = pe_value(vox + (m * P + s_rowpt[r]) * F, F, f, mode, g, coors[m * 4 + 1], coors[m * 4 + 2], mean_d);
        if (mode == PE_RADAR) v = pe_nan_to_num(v);
      }
      act[f * PS_RP + r] = v;
    }

    for (int l = 0; l < net.n; ++l) {
      const int K = net.K[l], C = net.C[l];
      const int ncg = C >> 2, nrg = PS_THREADS / ncg;   // column groups of 4, row groups of 8 (nrg >= 8: C <= 128)
      const int rg = tid % nrg, cg = tid / nrg;
      const bool active = cg < ncg && rg * 8 < rows;
      float acc[8][4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

      for (int kc = 0; kc < K; kc += PS_KC) {
        __syncthreads();   // act is complete; the previous chunk has been consumed
        const int kn = min(PS_KC, K - kc);
        const float4* src = reinterpret_cast<const float4*>(net.w[l] + (size_t)kc * C);
        for (int i = tid; i < kn * ncg; i += PS_THREADS) reinterpret_cast<float4*>(wl)[i] = src[i];
        __syncthreads();
        if (active) {
          const float* a = act + kc * PS_RP + rg * 8;
          const float* w = wl + cg * 4;
          for (int k = 0; k < kn; ++k) {
            const float4 a0 = *reinterpret_cast<const float4*>(a + k * PS_RP);
            const float4 a1 = *reinterpret_cast<const float4*>(a + k * PS_RP + 4);
            const float4 wv = *reinterpret_cast<const float4*>(w + k * C);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float wj[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], wj[j], acc[i][j]);
          }
        }
      }
      __syncthreads();   // every read of the layer's input is done: overwrite it
      if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = cg * 4 + j;
          const float s = net.scale[l][c], h = net.shift[l][c];
          float4 o0, o1;
          o0.x = fmaxf(fmaf(acc[0][j], s, h), 0.f); o0.y = fmaxf(fmaf(acc[1][j], s, h), 0.f);
          o0.z = fmaxf(fmaf(acc[2][j], s, h), 0.f); o0.w = fmaxf(fmaf(acc[3][j], s, h), 0.f);
          o1.x = fmaxf(fmaf(acc[4][j], s, h), 0.f); o1.y = fmaxf(fmaf(acc[5][j], s, h), 0.f);
          o1.z = fmaxf(fmaf(acc[6][j], s, h), 0.f); o1.w = fmaxf(fmaf(acc[7][j], s, h), 0.f);
          *reinterpret_cast<float4*>(act + c * PS_RP + rg * 8) = o0;
          *reinterpret_cast<float4*>(act + c * PS_RP + rg * 8 + 4) = o1;
        }
      }
      const bool last = l == net.n - 1;
      if (last || net.cat[l]) {
        __syncthreads();
        for (int idx = tid; idx < np * C; idx += PS_THREADS) {
          const int p = idx / C, c = idx - p * C;
          const int r0 = s_start[p], r1 = s_start[p + 1];
          float mx = act[c * PS_RP + r0];
          for (int r = r0 + 1; r < r1; ++r) mx = fmaxf(mx, act[c * PS_RP + r]);
          if (last) {
            out[(size_t)(m0 + p0 + p) * C + c] = mx;
          } else {
            for (int r = r0; r < r1; ++r) act[(C + c) * PS_RP + r] = mx;   // [x, max_over_P(x)]
          }
        }
        if (!last) {   // rows that only fill the last group of 8: keep them finite
          for (int idx = tid; idx < (rows8 - rows) * C; idx += PS_THREADS) {
            const int r = rows + idx / C, c = idx % C;
            act[(C + c) * PS_RP + r] = 0.f;
          }
        }
      }
    }
    __syncthreads();   // the row table and act are free for the next tile
    p0 = p1;
  }
}

// ---- scatter to the pseudo image ------------------------------------------------------------------------------------------
__device__ __forceinline__ long long ps_cell(const int* __restrict__ row, int B, int nx, int ny) {
  const int b = row[0], x = row[1], y = row[2];
  if (b < 0 || b >= B || x < 0 || x >= nx || y < 0 || y >= ny) return -1;
  return ((long long)b * nx + x) * ny + y;
}

__global__ __launch_bounds__(256) void pillar_scatter_winner_kernel(const int* __restrict__ coors, int M, int B, int nx, int ny,
                                                                    int* __restrict__ winner) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const long long cell = ps_cell(coors + (size_t)i * 4, B, nx, ny);
  if (cell >= 0) atomicMax(&winner[cell], i);
}

constexpr int PSC_CH = 8;   // channels per thread of the canvas pass

template <typename T>
__global__ __launch_bounds__(256) void pillar_scatter_canvas_kernel(const T* __restrict__ feats, const int* __restrict__ winner,
                                                                    int M, int C, int ncell, T* __restrict__ canvas) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= ncell) return;
  const int b = blockIdx.z, c0 = blockIdx.y * PSC_CH;
  const int w = winner[(size_t)b * ncell + cell];
  const bool hit = w >= 0 && w < M;
  T* dst = canvas + ((size_t)b * C + c0) * ncell + cell;
#pragma unroll
  for (int j = 0; j < PSC_CH; ++j)
    if (c0 + j < C) dst[(size_t)j * ncell] = hit ? feats[(size_t)w * C + c0 + j] : T(0);
}

template <typename T>
__global__ __launch_bounds__(256) void pillar_scatter_backward_kernel(const T* __restrict__ grad_canvas, const int* __restrict__ coors,
                                                                      const int* __restrict__ winner, long long total, int C, int B,
                                                                      int nx, int ny, T* __restrict__ grad_feats) {
  const long long ncell = (long long)nx * ny;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long row = e / C;
    const int c = (int)(e - row * C);
    const long long cell = ps_cell(coors + row * 4, B, nx, ny);
    T gval = T(0);
    if (cell >= 0 && winner[cell] == (int)row) {
      const long long b = cell / ncell;
      gval = grad_canvas[(b * C + c) * ncell + (cell - b * ncell)];
    }
    grad_feats[e] = gval;
  }
}

static unsigned pe_grid(long long total) {
  long long b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 16384 ? 16384 : b);
}

static PeGeom pe_geom(const float* p) {
  PeGeom g;
  g.vx = p[0]; g.vy = p[1]; g.xo = p[2]; g.yo = p[3];
  for (int d = 0; d < 3; ++d) { g.lo[d] = p[4 + d]; g.span[d] = p[7 + d]; }
  return g;
}

}  // namespace bevamd

using namespace bevamd;

extern "C" {

int bevamd_pillar_decorate(const float* voxels, const int* num_points, const int* coors, int num_pillars, int max_points,
                           int num_features, int mode, int with_distance, const float* geom, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(mode == PE_PILLAR || mode == PE_RADAR, "pillar_decorate: mode %d (0 pillar, 1 radar)", mode);
  BEVAMD_REQUIRE(num_pillars >= 0 && max_points >= 1 && num_features >= 3, "pillar_decorate: bad sizes (M %d, P %d, F %d)",
                 num_pillars, max_points, num_features);
  BEVAMD_REQUIRE(geom != nullptr, "pillar_decorate: geom is null");
  if (num_pillars == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(voxels && num_points && coors && out, "pillar_decorate: null buffer");
  const int Fo = mode == PE_RADAR ? num_features + 2 : num_features + 5 + (with_distance ? 1 : 0);
  const long long total = (long long)num_pillars * max_points * Fo;
  pillar_decorate_kernel<<<dim3(pe_grid(total)), dim3(256), 0, stream>>>(voxels, num_points, coors, total, max_points, num_features,
                                                                         Fo, mode, pe_geom(geom), out);
  BEVAMD_LAUNCH_CHECK("pillar_decorate");
  return BEVAMD_OK;
}

int bevamd_pillar_stack_forward(const float* voxels, const int* num_points, const int* coors, int num_pillars, int max_points,
                                int num_features, int mode, int with_distance, const float* geom, int num_layers,
                                const int* units, const void* const* weights, const void* const* scales,
                                const void* const* shifts, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(mode == PE_PILLAR || mode == PE_RADAR, "pillar_stack_forward: mode %d (0 pillar, 1 radar)", mode);
  BEVAMD_REQUIRE(num_pillars >= 0 && max_points >= 1 && num_features >= 3 && num_layers >= 1,
                 "pillar_stack_forward: bad sizes (M %d, P %d, F %d, layers %d)", num_pillars, max_points, num_features, num_layers);
  BEVAMD_REQUIRE(geom && units && weights && scales && shifts, "pillar_stack_forward: null host array");
  if (num_layers > PE_MAX_LAYERS || max_points > PE_MAX_P || num_features > PE_MAX_IN) {
    set_error("pillar_stack_forward: not supported (layers %d > %d, P %d > %d or F %d > %d)", num_layers, PE_MAX_LAYERS, max_points,
              PE_MAX_P, num_features, PE_MAX_IN);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  PsNet net;
  net.n = num_layers;
  const int Fo = mode == PE_RADAR ? num_features + 2 : num_features + 5 + (with_distance ? 1 : 0);
  int K = Fo;
  for (int l = 0; l < PE_MAX_LAYERS; ++l) {
    net.K[l] = net.C[l] = net.cat[l] = 0;
    net.w[l] = net.scale[l] = net.shift[l] = nullptr;
  }
  for (int l = 0; l < num_layers; ++l) {
    const int C = units[l];
    const bool cat = mode == PE_PILLAR && l < num_layers - 1;
    BEVAMD_REQUIRE(C >= 1, "pillar_stack_forward: layer %d has %d units", l, C);
    if (C > PE_MAX_WIDTH || (C & 3) || (cat && 2 * C > PE_MAX_WIDTH) || K > PE_MAX_WIDTH) {
      set_error("pillar_stack_forward: not supported (layer %d: %d -> %d; widths are multiples of 4 up to %d)", l, K, C, PE_MAX_WIDTH);
      return BEVAMD_ERR_UNSUPPORTED;
    }
    BEVAMD_REQUIRE(weights[l] && scales[l] && shifts[l], "pillar_stack_forward: layer %d has a null parameter", l);
    net.K[l] = K;
    net.C[l] = C;
    net.cat[l] = cat ? 1 : 0;
    net.w[l] = (const float*)weights[l];
    net.scale[l] = (const float*)scales[l];
    net.shift[l] = (const float*)shifts[l];
    K = cat ? 2 * C : C;
  }
  if (num_pillars == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(voxels && num_points && coors && out, "pillar_stack_forward: null buffer");
  pillar_stack_kernel<<<dim3(cdiv(num_pillars, PS_CHUNK)), dim3(PS_THREADS), 0, stream>>>(
      voxels, num_points, coors, num_pillars, max_points, num_features, Fo, mode, pe_geom(geom), net, out);
  BEVAMD_LAUNCH_CHECK("pillar_stack");
  return BEVAMD_OK;
}

int bevamd_pillar_scatter_forward(const void* feats, int dtype, const int* coors, int num_pillars, int channels, int batch_size,
                                  int nx, int ny, int* winner, void* canvas, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "pillar_scatter_forward: dtype %d (0 fp32, 1 fp16)", dtype);
  BEVAMD_REQUIRE(num_pillars >= 0 && channels >= 1 && batch_size >= 1 && nx >= 1 && ny >= 1 && batch_size <= 65535 &&
                     (long long)batch_size * nx * ny <= 0x7fffffffLL,
                 "pillar_scatter_forward: bad sizes (M %d, C %d, B %d, %d x %d)", num_pillars, channels, batch_size, nx, ny);
  BEVAMD_REQUIRE(winner && canvas && (num_pillars == 0 || (feats && coors)), "pillar_scatter_forward: null buffer");
  const int ncell = nx * ny;
  int rc = device_fill_u32((uint32_t*)winner, (size_t)batch_size * ncell, 0xffffffffu, stream);   // -1: nobody
  if (rc) return rc;
  if (num_pillars > 0) {
    pillar_scatter_winner_kernel<<<dim3(cdiv(num_pillars, 256)), dim3(256), 0, stream>>>(coors, num_pillars, batch_size, nx, ny, winner);
    BEVAMD_LAUNCH_CHECK("pillar_scatter_winner");
  }
  const dim3 grid(cdiv(ncell, 256), cdiv(channels, PSC_CH), batch_size);
  BEVAMD_REQUIRE(grid.y <= 65535, "pillar_scatter_forward: too many channels (%d)", channels);
  if (dtype == 0)
    pillar_scatter_canvas_kernel<float><<<grid, dim3(256), 0, stream>>>((const float*)feats, winner, num_pillars, channels, ncell, (float*)canvas);
  else
    pillar_scatter_canvas_kernel<_Float16><<<grid, dim3(256), 0, stream>>>((const _Float16*)feats, winner, num_pillars, channels, ncell, (_Float16*)canvas);
  BEVAMD_LAUNCH_CHECK("pillar_scatter_canvas");
  return BEVAMD_OK;
}

int bevamd_pillar_scatter_backward(const void* grad_canvas, int dtype, const int* coors, const int* winner, int num_pillars,
                                   int channels, int batch_size, int nx, int ny, void* grad_feats, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(dtype == 0 || dtype == 1, "pillar_scatter_backward: dtype %d (0 fp32, 1 fp16)", dtype);
  BEVAMD_REQUIRE(num_pillars >= 0 && channels >= 1 && batch_size >= 1 && nx >= 1 && ny >= 1 &&
                     (long long)batch_size * nx * ny <= 0x7fffffffLL,
                 "pillar_scatter_backward: bad sizes (M %d, C %d, B %d, %d x %d)", num_pillars, channels, batch_size, nx, ny);
  if (num_pillars == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(grad_canvas && coors && winner && grad_feats, "pillar_scatter_backward: null buffer");
  const long long total = (long long)num_pillars * channels;
  if (dtype == 0)
    pillar_scatter_backward_kernel<float><<<dim3(pe_grid(total)), dim3(256), 0, stream>>>((const float*)grad_canvas, coors, winner, total, channels,
                                                                                       batch_size, nx, ny, (float*)grad_feats);
  else
    pillar_scatter_backward_kernel<_Float16><<<dim3(pe_grid(total)), dim3(256), 0, stream>>>((const _Float16*)grad_canvas, coors, winner, total,
                                                                                          channels, batch_size, nx, ny, (_Float16*)grad_feats);
  BEVAMD_LAUNCH_CHECK("pillar_scatter_backward");
  return BEVAMD_OK;
}

}  // extern "C"
