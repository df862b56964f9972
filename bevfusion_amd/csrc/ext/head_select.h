// Top-K selection shared by the head-end units (head_ends.hip: TransFusion proposals; centerpoint_ends.hip: CenterHead's
// per-task top-K).  Candidates are 64-bit keys, score bits high and the complemented flat index low, so that key order IS the
// defined order: descending score, equal scores in ascending flat index.
#pragma once

#include "common.h"

#include <math.h>

namespace bevamd {
namespace head {

constexpr int HE_MAX_K = 1024;       // proposals per sample, rows per NMS segment
constexpr int HE_SEL_THREADS = 1024;
constexpr int HE_BINS = 2048;        // 11-bit digits

__device__ __forceinline__ float he_sigmoid(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// One workgroup of HE_SEL_THREADS threads selects the K (<= HE_MAX_K) largest of the n DISTINCT keys cand[0 .. n) and hands them to
// write(position, key) in descending order: an MSB-first radix select (11-bit digits, LDS histogram) finds the K-th key, the keys
// at or above it are collected and rank-sorted in LDS.  When n < K, the flat indices below min(2K, chw) that no candidate names
// follow in ascending order as keys with zero score bits (at least K - n of them exist).
template <typename Write>
__device__ __forceinline__ void he_select_segment(const unsigned long long* __restrict__ cand, unsigned n, unsigned chw, int K,
                                                  Write write) {
  __shared__ unsigned hist[HE_BINS];
  __shared__ unsigned long long skey[HE_MAX_K];
  __shared__ unsigned char flag[2 * HE_MAX_K];
  __shared__ unsigned s_wsum[HE_SEL_THREADS / 64];
  __shared__ unsigned s_digit, s_rem, s_nsel;

  const int tid = threadIdx.x;

  // the K-th largest key (keys are distinct): MSB-first radix select, 64 = 5 * 11 + 9 bits
  unsigned long long kth = 0;
  if (n > (unsigned)K) {
    unsigned rem = (unsigned)K;
    unsigned long long prefix = 0;
    int hi = 64;   // bits [hi, 64) of the K-th key are known
    while (hi > 0) {
      const int bits = hi >= 11 ? 11 : hi;
      const int shift = hi - bits;
      const unsigned dmask = (1u << bits) - 1u;
      for (int i = tid; i < HE_BINS; i += HE_SEL_THREADS) hist[i] = 0;
      __syncthreads();
      for (unsigned i = tid; i < n; i += HE_SEL_THREADS) {
        const unsigned long long key = cand[i];
        if (hi == 64 || (key >> hi) == (prefix >> hi)) atomicAdd(&hist[(unsigned)(key >> shift) & dmask], 1u);
      }
      __syncthreads();
      if (tid < 64) {   // wave 0: lane l owns the 32 bins below 2047 - 32 l, walked downwards
        const int top = HE_BINS - 1 - 32 * tid;
        unsigned sum = 0;
        for (int j = 0; j < 32; ++j) sum += hist[top - j];
        const unsigned incl = wave_inclusive_scan(sum), excl = incl - sum;
        if (excl < rem && rem <= incl) {
          unsigned acc = excl;
          for (int j = 0; j < 32; ++j) {
            const unsigned h = hist[top - j];
            if (acc + h >= rem) {
              s_digit = (unsigned)(top - j);
              s_rem = rem - acc;
              break;
            }
            acc += h;
          }
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)s_digit << shift;
      rem = s_rem;
      hi = shift;
    }
    kth = prefix;
  }

  if (tid == 0) s_nsel = 0;
  __syncthreads();
  for (unsigned i = tid; i < n; i += HE_SEL_THREADS) {
    const unsigned long long key = cand[i];
    if (key >= kth) {
      const unsigned p = atomicAdd(&s_nsel, 1u);
      if (p < (unsigned)HE_MAX_K) skey[p] = key;
    }
  }
  __syncthreads();
  const unsigned nsel = min(s_nsel, (unsigned)K);   // min(n, K)

  if ((unsigned)tid < nsel) {   // rank sort, descending
    const unsigned long long mine = skey[tid];
    unsigned rank = 0;
    for (unsigned j = 0; j < nsel; ++j) rank += skey[j] > mine ? 1u : 0u;
    write(rank, mine);
  }

  if (nsel < (unsigned)K) {   // block-uniform.  Zeros of the suppressed map in ascending flat index: here n < K, so n = nsel
    const unsigned lim = min(2u * (unsigned)K, chw);   // at least K - n cells below lim are not candidates
    for (int i = tid; i < 2 * HE_MAX_K; i += HE_SEL_THREADS) flag[i] = 0;
    __syncthreads();
    for (unsigned i = tid; i < n; i += HE_SEL_THREADS) {
      const unsigned flat = ~(unsigned)cand[i];
      if (flat < lim) flag[flat] = 1;
    }
    __syncthreads();
    const unsigned f0 = 2u * tid, f1 = f0 + 1u;
    const unsigned z0 = (f0 < lim && !flag[f0]) ? 1u : 0u, z1 = (f1 < lim && !flag[f1]) ? 1u : 0u;
    const unsigned incl = wave_inclusive_scan(z0 + z1);
    if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
    __syncthreads();
    unsigned pos = nsel + incl - (z0 + z1);
    for (int w = 0; w < (tid >> 6); ++w) pos += s_wsum[w];
    if (z0 && pos < (unsigned)K) write(pos, (unsigned long long)(~f0));
    pos += z0;
    if (z1 && pos < (unsigned)K) write(pos, (unsigned long long)(~f1));
  }
}

}  // namespace head
}  // namespace bevamd
