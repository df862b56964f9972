// Fused multi-head attention of the TransFusion decoder layer, gfx950: softmax(q k^T / 4) v for heads of dimension 16.
//
// Replaces (reference):
//   mmdet3d/models/utils/transformer.py:244-493  multi_head_attention_forward: the [heads, L, S] fp32 logits written and read again
//                                                for the softmax and for dropout, head-averaged weights nobody reads, two torch.equal
//
// Native formulation.  The logits never reach memory; every product runs on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains), the head
// dimension 16 being one tile edge.  q is scaled by 0.25 on load (a power of two: the same bits as scaling the logits).
//   forward  * mha_fwd_kernel     grid (splits, ceil(L / 64), B * H), 4 waves; a wave owns 16 queries of one head and walks its
//                                 split's keys 64 at a time.  S^T = K Q^T puts the query on the lane and 16 keys in its registers,
//                                 so the row maximum is 15 fmax and two cross-lane steps, and exp(S^T - m) is already the B operand
//                                 of O^T += V^T P^T: nothing crosses LDS.  Online softmax: running (max, sum, O^T) per query.
//            * mha_merge_kernel   merges the splits' (max, sum, partial out) in split order into out and lse.
//   backward * mha_delta_kernel   delta = rowsum(dout * out)
//            * mha_bwd_kernel     grid (key blocks, B * H), 4 waves x 64 keys per chunk; a workgroup owns its keys, loops over the
//                                 query tiles and writes its dk / dv rows once.  P = exp((Q K^T - max) - log sum) from lse kept in two
//                                 terms (a maximum of 96 would cost lse five digits).  S and dP = dO V^T with the key on the
//                                 lane are the B operands of dV^T += dO^T P and dK^T += Q^T dS; only dS crosses LDS, for
//                                 dQ += dS K, which the four waves sum in LDS and store into the key block's partial buffer.
//            * mha_dq_sum_kernel  sums the key blocks' partial dq in block order.
// No floating-point atomics: every sum has a fixed order, and the split / block counts depend on (B, H, L, S) only.
// Dropout is a counter hash of (seed, b * H + h, query, key) in registers, the same in both directions, applied to the normalised
// weights: the row sum uses the undropped weights, kept weights are scaled by 1 / (1 - p).
#include <hip/hip_fp16.h>

#include "common.h"

namespace bevamd {
namespace mha {

constexpr int MH_D = 16;               // head dimension, the only one
constexpr int MH_MAX_HEADS = 16;
constexpr int MH_MAX_L = 1024;
constexpr int MH_MAX_S = 1 << 20;
constexpr int MH_THREADS = 256;        // 4 waves
constexpr int MH_QROWS = 64;           // queries of a forward workgroup: 16 per wave
constexpr int MH_KSTEP = 64;           // keys of one forward iteration; a split is a multiple of it
constexpr int MH_FWD_WAVES = 8192;     // what the forward split count aims at (8 waves per SIMD)
constexpr int MH_MAX_SPLITS = 64;
constexpr int MH_BWD_KEYS = 256;       // keys of one backward chunk: 64 per wave
constexpr int MH_BWD_BLOCKS = 2048;    // workgroups the backward block count aims at
constexpr int MH_MAX_BWD_BLOCKS = 256;
constexpr int MH_DS_PITCH = 20;        // floats per row of a dS tile in LDS: float4 reads stay aligned, rows spread over banks

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Plan {
  int splits, split_keys;              // forward
  int blocks, chunks;                  // backward: key blocks, chunks of MH_BWD_KEYS keys per block
};

static bool shape_ok(int B, int H, int L, int S) {
  return B >= 1 && B <= 65535 / MH_MAX_HEADS && H >= 1 && H <= MH_MAX_HEADS && L >= 1 && L <= MH_MAX_L && S >= 1 && S <= MH_MAX_S;
}

static Plan make_plan(int B, int H, int L, int S) {
  Plan p;
  const long long waves = (long long)B * H * cdiv(L, 16);
  long long want = (MH_FWD_WAVES + waves - 1) / waves;
  if (want > MH_MAX_SPLITS) want = MH_MAX_SPLITS;
  if (want < 1) want = 1;
  p.split_keys = cdiv(cdiv(S, want), MH_KSTEP) * MH_KSTEP;
  p.splits = cdiv(S, p.split_keys);                       // every split has at least one key
  const int total_chunks = cdiv(S, MH_BWD_KEYS);
  long long blocks = (MH_BWD_BLOCKS + (long long)B * H - 1) / ((long long)B * H);
  if (blocks > MH_MAX_BWD_BLOCKS) blocks = MH_MAX_BWD_BLOCKS;
  if (blocks > total_chunks) blocks = total_chunks;
  p.chunks = cdiv(total_chunks, blocks);
  p.blocks = cdiv(total_chunks, p.chunks);
  return p;
}

static size_t fwd_bytes(const Plan& p, int B, int H, int L) {
  const size_t rows = (size_t)p.splits * B * H * L;
  return align_up(rows * MH_D * sizeof(float), 256) + 2 * align_up(rows * sizeof(float), 256);
}

static size_t bwd_bytes(const Plan& p, int B, int H, int L) {
  return align_up((size_t)B * H * L * sizeof(float), 256) + align_up((size_t)p.blocks * B * L * H * MH_D * sizeof(float), 256);
}

// ---- loads: fp16 inputs are widened in registers -----------------------------------------------------------------------------------
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const __half* p) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  const __half2 a = *reinterpret_cast<const __half2*>(&w.x), b = *reinterpret_cast<const __half2*>(&w.y);
  const float2 fa = __half22float2(a), fb = __half22float2(b);
  return make_float4(fa.x, fa.y, fb.x, fb.y);
}
__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(__half* p, float v) { *p = __float2half(v); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float elem(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// ---- dropout: a counter hash (mirrored by decoder._dropout_keep_host) ----------------------------------------------------------------
__device__ __host__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the two words of a (seed, head, query) row
__device__ __forceinline__ uint2 drop_row(unsigned long long seed, int bh, int query) {
  const unsigned long long z = mix64(mix64(seed) + (((unsigned long long)bh << 10) | (unsigned)query));
  return make_uint2((unsigned)z, (unsigned)(z >> 32));
}
__device__ __forceinline__ bool drop_keep(uint2 row, int key, unsigned threshold) {
  unsigned x = (unsigned)key * 0x9E3779B1u + row.x;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x += row.y;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x >= threshold;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <typename T, bool DROP>
__global__ __launch_bounds__(MH_THREADS) void mha_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                             int H, int L, int S, int split_keys, unsigned threshold, float keep_scale,
                                                             unsigned long long seed, float* __restrict__ po, float* __restrict__ pm,
                                                             float* __restrict__ pl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qt = blockIdx.y * (MH_QROWS / 16) + wave;
  if (qt * 16 >= L) return;                                  // no barrier in this kernel
  const int bh = blockIdx.z, b = bh / H, h = bh - b * H, split = blockIdx.x;
  const int c = lane & 15, g = lane >> 4, E = H * MH_D;
  const int query = qt * 16 + c, qrow = query < L ? query : L - 1;
  float4 qf = load4(q + ((size_t)b * L + qrow) * E + h * MH_D + g * 4);
  qf.x *= 0.25f, qf.y *= 0.25f, qf.z *= 0.25f, qf.w *= 0.25f;
  const int k0 = split * split_keys, k1 = k0 + split_keys < S ? k0 + split_keys : S;
  const T* kb = k + (size_t)b * S * E + h * MH_D;
  const T* vb = v + (size_t)b * S * E + h * MH_D;
  uint2 row = make_uint2(0u, 0u);
  if (DROP) row = drop_row(seed, bh, query);

  float m = -INFINITY, sum = 0.f;
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
  for (int kk = k0; kk < k1; kk += MH_KSTEP) {
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                            // S^T[key][query] of 16 keys: row = key g * 4 + r, column = query c
      int key = kk + j * 16 + c;
      key = key < S ? key : S - 1;
      const float4 kf = load4(kb + (size_t)key * E + g * 4);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = mfma4(kf.x, qf.x, acc);
      acc = mfma4(kf.y, qf.y, acc);
      acc = mfma4(kf.z, qf.z, acc);
      acc = mfma4(kf.w, qf.w, acc);
      s[j] = acc;
    }
    float vv[4][4];
    float mx = m;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kk + j * 16 + g * 4 + r;
        const bool live = key < k1;
        vv[j][r] = load1(vb + (size_t)(live ? key : k1 - 1) * E + c);
        if (!live) vv[j][r] = 0.f, s[j][r] = -INFINITY;
        mx = fmaxf(mx, s[j][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float rescale = expf(m - mx);                      // first tile: exp(-inf) = 0 on zeros
    m = mx;
    sum *= rescale;
    o0 *= rescale;
    o1 *= rescale;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = expf(s[j][r] - mx);
        sum += p;
        if (DROP) p = drop_keep(row, kk + j * 16 + g * 4 + r, threshold) ? p * keep_scale : 0.f;
        if (j & 1)
          o1 = mfma4(vv[j][r], p, o1);                       // O^T[d][query] += V^T[d][key] P^T[key][query]
        else
          o0 = mfma4(vv[j][r], p, o0);
      }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (query < L) {
    const size_t at = ((size_t)split * gridDim.z + bh) * L + query;
    const f32x4 o = o0 + o1;
    *reinterpret_cast<float4*>(po + at * MH_D + g * 4) = make_float4(o[0], o[1], o[2], o[3]);
    if (g == 0) pm[at] = m, pl[at] = sum;
  }
}

template <typename T>
__global__ __launch_bounds__(MH_THREADS) void mha_merge_kernel(const float* __restrict__ po, const float* __restrict__ pm,
                                                               const float* __restrict__ pl, int splits, int B, int H, int L,
                                                               T* __restrict__ out, float* __restrict__ lse, float* __restrict__ stats) {
  const size_t rows = (size_t)B * H * L;
  const size_t at = (size_t)blockIdx.x * MH_THREADS + threadIdx.x;
  const size_t rowi = at / MH_D;
  const int d = (int)(at % MH_D);
  if (rowi >= rows) return;
  float m = -INFINITY;
  for (int s = 0; s < splits; ++s) m = fmaxf(m, pm[s * rows + rowi]);
  float sum = 0.f, acc = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float w = expf(pm[s * rows + rowi] - m);
    sum += pl[s * rows + rowi] * w;
    acc += po[(s * rows + rowi) * MH_D + d] * w;
  }
  const int query = (int)(rowi % L);
  const size_t bh = rowi / L;
  const int h = (int)(bh % H);
  const size_t b = bh / H;
  store1(out + (b * L + query) * (size_t)(H * MH_D) + h * MH_D + d, acc / sum);
  if (d == 0) {
    const float logsum = logf(sum);
    lse[rowi] = m + logsum;
    if (stats) stats[rowi] = m, stats[rows + rowi] = logsum;  // lse in two terms: the sum loses nothing to a large maximum
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MH_THREADS) void mha_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout, int B, int H,
                                                               int L, float* __restrict__ delta) {
  const size_t rows = (size_t)B * H * L;
  const size_t rowi = (size_t)blockIdx.x * MH_THREADS + threadIdx.x;
  if (rowi >= rows) return;
  const int query = (int)(rowi % L);
  const size_t bh = rowi / L;
  const int h = (int)(bh % H);
  const size_t b = bh / H, at = (b * L + query) * (size_t)(H * MH_D) + h * MH_D;
  float4 a[4], g[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = load4(out + at + i * 4), g[i] = load4(dout + at + i * 4);
  // the order of the backward kernel's dP = dO V^T chain (d = 0, 4, 8, 12, 1, 5, ...): where one weight is 1 and out is that value
  // row, dP - delta is 0 bit for bit, as it is in the reference's softmax backward
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(elem(g[j], i), elem(a[j], i), acc);
  delta[rowi] = acc;
}

template <bool DROP>
__global__ __launch_bounds__(MH_THREADS) void mha_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, const float* __restrict__ stats,
                                                             const float* __restrict__ delta, const float* __restrict__ dout, int B, int H,
                                                             int L, int S, int chunks, unsigned threshold, float keep_scale,
                                                             unsigned long long seed, float* __restrict__ dqp, float* __restrict__ dk,
                                                             float* __restrict__ dv) {
  __shared__ float ds_lds[4][4][16 * MH_DS_PITCH];           // [wave][key tile][query][key]
  __shared__ float dq_lds[4][16 * 16];                       // [wave][query][d]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int c = lane & 15, g = lane >> 4, E = H * MH_D;
  const float* qb = q + (size_t)b * L * E + h * MH_D;
  const float* dob = dout + (size_t)b * L * E + h * MH_D;
  const float* kb = k + (size_t)b * S * E + h * MH_D;
  const float* vb = v + (size_t)b * S * E + h * MH_D;
  const float* maxb = stats + (size_t)bh * L;              // lse in two terms: the row maximum and the log of the row sum
  const float* logsumb = maxb + (size_t)B * H * L;
  const float* deltab = delta + (size_t)bh * L;
  float* dqb = dqp + ((size_t)blockIdx.x * B + b) * L * E + h * MH_D;
  const int qtiles = (L + 15) / 16;

  for (int chunk = 0; chunk < chunks; ++chunk) {
    const int kw = (blockIdx.x * chunks + chunk) * MH_BWD_KEYS + wave * 64;   // a workgroup past S still meets the barriers
    float4 kB[4], vB[4];                                     // K^T, V^T [d = g * 4 + i][key c]: B operands of S and dP
    float kD[4][4];                                          // K[key g * 4 + i][d c]: B operand of dQ
    f32x4 dkT[4], dvT[4];                                    // dK^T, dV^T [d = g * 4 + r][key c]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int key = kw + t * 16 + c;
      key = key < S ? key : S - 1;
      kB[t] = load4(kb + (size_t)key * E + g * 4);
      vB[t] = load4(vb + (size_t)key * E + g * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int kr = kw + t * 16 + g * 4 + i;
        kr = kr < S ? kr : S - 1;
        kD[t][i] = kb[(size_t)kr * E + c];
      }
      dkT[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dvT[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int qt = 0; qt < qtiles; ++qt) {
      const int qc = qt * 16 + c, qcc = qc < L ? qc : L - 1;
      float4 qA = load4(qb + (size_t)qcc * E + g * 4);       // Q[query c][d = g * 4 + i] / 4: A operand of S
      qA.x *= 0.25f, qA.y *= 0.25f, qA.z *= 0.25f, qA.w *= 0.25f;
      const float4 doA = load4(dob + (size_t)qcc * E + g * 4);
      float qT[4], doT[4], rmax[4], rlog[4], dl[4];                   // Q^T / 4, dO^T [d c][query g * 4 + i]: A operands of dK^T, dV^T
      uint2 row[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qr = qt * 16 + g * 4 + i, qrc = qr < L ? qr : L - 1;
        qT[i] = qr < L ? 0.25f * qb[(size_t)qrc * E + c] : 0.f;
        doT[i] = qr < L ? dob[(size_t)qrc * E + c] : 0.f;
        rmax[i] = maxb[qrc];
        rlog[i] = logsumb[qrc];
        dl[i] = deltab[qrc];
        if (DROP) row[i] = drop_row(seed, bh, qr);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x4 sa = {0.f, 0.f, 0.f, 0.f};                     // S[query g * 4 + r][key c]: the forward's chain, bit for bit
        f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sa = mfma4(elem(qA, i), elem(kB[t], i), sa);
          dp = mfma4(elem(doA, i), elem(vB[t], i), dp);
        }
        const int key = kw + t * 16 + c;
        f32x4 pd, dsv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = key < S && qt * 16 + g * 4 + r < L;
          const float p = live ? expf((sa[r] - rmax[r]) - rlog[r]) : 0.f;
          float w = p, dpr = dp[r];
          if (DROP) {
            const bool keep = drop_keep(row[r], key, threshold);
            w = keep ? p * keep_scale : 0.f;
            dpr = keep ? dpr * keep_scale : 0.f;
          }
          pd[r] = w;
          dsv[r] = live ? p * (dpr - dl[r]) : 0.f;
          ds_lds[wave][t][(g * 4 + r) * MH_DS_PITCH + c] = dsv[r];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dvT[t] = mfma4(doT[i], pd[i], dvT[t]);             // dV^T[d][key] += dO^T[d][query] P[query][key]
          dkT[t] = mfma4(qT[i], dsv[i], dkT[t]);             // dK^T[d][key] += Q^T[d][query] dS[query][key] (/ 4 inside qT)
        }
      }
      __syncthreads();
      f32x4 dq = {0.f, 0.f, 0.f, 0.f};                       // dQ[query g * 4 + r][d c]
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float4 a = *reinterpret_cast<const float4*>(&ds_lds[wave][t][c * MH_DS_PITCH + g * 4]);   // dS[query c][key g * 4 + i]
#pragma unroll
        for (int i = 0; i < 4; ++i) dq = mfma4(elem(a, i), kD[t][i], dq);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) dq_lds[wave][(g * 4 + r) * 16 + c] = dq[r];
      __syncthreads();
      {
        const int e = threadIdx.x, qr = qt * 16 + (e >> 4);
        const float total = (dq_lds[0][e] + dq_lds[1][e]) + (dq_lds[2][e] + dq_lds[3][e]);
        if (qr < L) {
          float* at = dqb + (size_t)qr * E + (e & 15);
          *at = chunk ? *at + total : total;                 // the same thread every chunk: program order
        }
      }                                                      // the next tile's first barrier stands between these reads and its writes
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = kw + t * 16 + c;
      if (key < S) {
        const size_t at = ((size_t)b * S + key) * E + h * MH_D + g * 4;
        *reinterpret_cast<float4*>(dk + at) = make_float4(dkT[t][0], dkT[t][1], dkT[t][2], dkT[t][3]);
        *reinterpret_cast<float4*>(dv + at) = make_float4(dvT[t][0], dvT[t][1], dvT[t][2], dvT[t][3]);
      }
    }
  }
}

__global__ __launch_bounds__(MH_THREADS) void mha_dq_sum_kernel(const float* __restrict__ dqp, int blocks, size_t n, float* __restrict__ dq) {
  const size_t at = ((size_t)blockIdx.x * MH_THREADS + threadIdx.x) * 4;
  if (at >= n) return;
  float4 acc = load4(dqp + at);
  for (int s = 1; s < blocks; ++s) {
    const float4 a = load4(dqp + s * n + at);
    acc.x += a.x, acc.y += a.y, acc.z += a.z, acc.w += a.w;
  }
  *reinterpret_cast<float4*>(dq + at) = make_float4(0.25f * acc.x, 0.25f * acc.y, 0.25f * acc.z, 0.25f * acc.w);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int check_dropout(const char* what, double p) {
  if (!(p >= 0.0 && p < 1.0)) {
    set_error("%s: dropout_p %g (0 <= p < 1)", what, p);
    return BEVAMD_ERR_INVALID_ARG;
  }
  return BEVAMD_OK;
}

static unsigned drop_threshold(double p) {
  const double t = p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}

}  // namespace mha
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::mha;

extern "C" {

size_t bevamd_mha_workspace_bytes(int B, int H, int L, int S) {
  if (!shape_ok(B, H, L, S)) return 0;
  const Plan p = make_plan(B, H, L, S);
  const size_t f = fwd_bytes(p, B, H, L), w = bwd_bytes(p, B, H, L);
  return f > w ? f : w;
}

int bevamd_mha_plan(int B, int H, int L, int S, int* plan4) {
  BEVAMD_REQUIRE(shape_ok(B, H, L, S) && plan4,
                 "mha_plan: bad sizes (B %d (1 .. 4095), H %d (1 .. 16), L %d (1 .. 1024), S %d (1 .. 2^20))", B, H, L, S);
  const Plan p = make_plan(B, H, L, S);
  plan4[0] = p.splits, plan4[1] = p.split_keys, plan4[2] = p.blocks, plan4[3] = p.chunks * MH_BWD_KEYS;
  return BEVAMD_OK;
}

int bevamd_mha_forward(const void* q, const void* k, const void* v, int B, int H, int L, int S, int dtype, double dropout_p,
                       unsigned long long seed, void* out, float* lse, float* stats, void* workspace, size_t workspace_bytes,
                       void* stream) {
  BEVAMD_REQUIRE(shape_ok(B, H, L, S), "mha_forward: bad sizes (B %d (1 .. 4095), H %d (1 .. 16), L %d (1 .. 1024), S %d (1 .. 2^20))", B,
                 H, L, S);
  if (dtype != 0 && dtype != 1) {
    set_error("mha_forward: dtype %d (0 fp32, 1 fp16)", dtype);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (int rc = check_dropout("mha_forward", dropout_p)) return rc;
  BEVAMD_REQUIRE(q && k && v && out && lse && workspace, "mha_forward: null pointer");
  BEVAMD_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(workspace),
                 "mha_forward: q, k, v, out and the workspace must be 16-byte aligned");
  const Plan p = make_plan(B, H, L, S);
  if (workspace_bytes < fwd_bytes(p, B, H, L)) {
    set_error("mha_forward: workspace of %zu bytes, %zu needed", workspace_bytes, fwd_bytes(p, B, H, L));
    return BEVAMD_ERR_WORKSPACE;
  }
  const size_t rows = (size_t)p.splits * B * H * L;
  Carver cv(workspace, workspace_bytes);
  float* po = cv.take<float>(rows * MH_D);
  float* pm = cv.take<float>(rows);
  float* pl = cv.take<float>(rows);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(p.splits, cdiv(L, MH_QROWS), B * H), block(MH_THREADS);
  const bool drop = dropout_p > 0.0;
  const unsigned thr = drop_threshold(dropout_p);
  const float scale = (float)(1.0 / (1.0 - dropout_p));
#define MHA_FWD(T, DROP)                                                                                                              \
  hipLaunchKernelGGL((mha_fwd_kernel<T, DROP>), grid, block, 0, s, (const T*)q, (const T*)k, (const T*)v, H, L, S, p.split_keys, thr, \
                     scale, seed, po, pm, pl)
  if (dtype == 0) {
    if (drop) {
      MHA_FWD(float, true);
    } else {
      MHA_FWD(float, false);
    }
  } else {
    if (drop) {
      MHA_FWD(__half, true);
    } else {
      MHA_FWD(__half, false);
    }
  }
#undef MHA_FWD
  BEVAMD_LAUNCH_CHECK("mha_forward");
  const int merge_blocks = cdiv((long long)B * H * L * MH_D, MH_THREADS);
  if (dtype == 0)
    hipLaunchKernelGGL((mha_merge_kernel<float>), dim3(merge_blocks), block, 0, s, po, pm, pl, p.splits, B, H, L, (float*)out, lse,
                       stats);
  else
    hipLaunchKernelGGL((mha_merge_kernel<__half>), dim3(merge_blocks), block, 0, s, po, pm, pl, p.splits, B, H, L, (__half*)out, lse,
                       stats);
  BEVAMD_LAUNCH_CHECK("mha_forward merge");
  return BEVAMD_OK;
}

int bevamd_mha_backward(const float* q, const float* k, const float* v, const float* out, const float* stats, const float* dout, int B,
                        int H, int L, int S, double dropout_p, unsigned long long seed, float* dq, float* dk, float* dv, void* workspace,
                        size_t workspace_bytes, void* stream) {
  BEVAMD_REQUIRE(shape_ok(B, H, L, S), "mha_backward: bad sizes (B %d (1 .. 4095), H %d (1 .. 16), L %d (1 .. 1024), S %d (1 .. 2^20))", B,
                 H, L, S);
  if (int rc = check_dropout("mha_backward", dropout_p)) return rc;
  BEVAMD_REQUIRE(q && k && v && out && stats && dout && dq && dk && dv && workspace, "mha_backward: null pointer");
  BEVAMD_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) && aligned16(dq) && aligned16(dk) &&
                     aligned16(dv) && aligned16(workspace),
                 "mha_backward: the tensors and the workspace must be 16-byte aligned");
  const Plan p = make_plan(B, H, L, S);
  if (workspace_bytes < bwd_bytes(p, B, H, L)) {
    set_error("mha_backward: workspace of %zu bytes, %zu needed", workspace_bytes, bwd_bytes(p, B, H, L));
    return BEVAMD_ERR_WORKSPACE;
  }
  const size_t rows = (size_t)B * H * L, n = (size_t)B * L * H * MH_D;
  Carver cv(workspace, workspace_bytes);
  float* delta = cv.take<float>(rows);
  float* dqp = cv.take<float>((size_t)p.blocks * n);
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(MH_THREADS);
  hipLaunchKernelGGL(mha_delta_kernel, dim3(cdiv((long long)rows, MH_THREADS)), block, 0, s, out, dout, B, H, L, delta);
  BEVAMD_LAUNCH_CHECK("mha_backward delta");
  const dim3 grid(p.blocks, B * H);
  const unsigned thr = drop_threshold(dropout_p);
  const float scale = (float)(1.0 / (1.0 - dropout_p));
  if (dropout_p > 0.0)
    hipLaunchKernelGGL((mha_bwd_kernel<true>), grid, block, 0, s, q, k, v, stats, delta, dout, B, H, L, S, p.chunks, thr, scale, seed, dqp,
                       dk, dv);
  else
    hipLaunchKernelGGL((mha_bwd_kernel<false>), grid, block, 0, s, q, k, v, stats, delta, dout, B, H, L, S, p.chunks, thr, scale, seed, dqp,
                       dk, dv);
  BEVAMD_LAUNCH_CHECK("mha_backward");
  hipLaunchKernelGGL(mha_dq_sum_kernel, dim3(cdiv((long long)(n / 4), MH_THREADS)), block, 0, s, dqp, p.blocks, n, dq);
  BEVAMD_LAUNCH_CHECK("mha_backward dq sum");
  return BEVAMD_OK;
}

}  // extern "C"
