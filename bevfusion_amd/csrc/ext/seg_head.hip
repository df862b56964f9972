// Map segmentation metrics, gfx950: the tp / fp / fn counts of every class and threshold.
//
// Replaces (reference):
//   mmdet3d/datasets/nuscenes_dataset.py:498-530  evaluate_map: per sample a [K, H*W, 7] boolean tensor materialised three times
//                                                 (pred & label, pred & ~label, ~pred & label) and summed, about ten launches a sample
//
// Native formulation, all samples in one call:
//   * iou_zero_kernel    counts zeroed inside the call: a replay starts clean;
//   * iou_count_kernel   grid (workgroups per class, classes): every thread keeps, per threshold, how many of its cells have
//                        pred >= threshold (fp32) with and without the label, and how many are labelled; waves reduce by shuffle and
//                        lane 0 adds the wave's totals with 64-bit integer atomics (exact, independent of arrival order);
//                        fn = labelled - tp.  Each prediction and label is read once for all thresholds.
// bevamd_seg_iou_counts: 2 launches for any number of samples, classes and thresholds (up to 16).  No workspace, nothing read back.
#include "common.h"

namespace bevamd {
namespace seg_head {

constexpr int SG_THREADS = 256;
constexpr int SG_MAX_GRID = 2048;          // workgroups of a launch
constexpr int SG_MAX_THRESHOLDS = 16;
constexpr int SG_CELLS_PER_THREAD = 8;     // what the grid is sized for before the cap

__global__ __launch_bounds__(SG_THREADS) void iou_zero_kernel(unsigned long long* __restrict__ counts, int n) {
  for (int i = blockIdx.x * SG_THREADS + threadIdx.x; i < n; i += gridDim.x * SG_THREADS) counts[i] = 0ull;
}

template <typename Tl>
__global__ __launch_bounds__(SG_THREADS) void iou_count_kernel(const float* __restrict__ pred, const Tl* __restrict__ label, int samples,
                                                               int classes, long long hw, const float* __restrict__ thresholds,
                                                               int num_thresholds, unsigned long long* __restrict__ counts) {
  const int k = blockIdx.y;
  float thr[SG_MAX_THRESHOLDS];
#pragma unroll
  for (int t = 0; t < SG_MAX_THRESHOLDS; ++t) thr[t] = thresholds[t < num_thresholds ? t : 0];
  int with[SG_MAX_THRESHOLDS], without[SG_MAX_THRESHOLDS], labelled = 0;
#pragma unroll
  for (int t = 0; t < SG_MAX_THRESHOLDS; ++t) with[t] = without[t] = 0;
  const long long n = hw * samples, stride = (long long)gridDim.x * SG_THREADS;
  for (long long v = (long long)blockIdx.x * SG_THREADS + threadIdx.x; v < n; v += stride) {
    const long long s = v / hw, at = (s * classes + k) * hw + (v - s * hw);
    const float pv = pred[at];
    const int l = label[at] != (Tl)0 ? 1 : 0;
    labelled += l;
#pragma unroll
    for (int t = 0; t < SG_MAX_THRESHOLDS; ++t) {
      const int hit = pv >= thr[t] ? 1 : 0;
      with[t] += hit & l;
      without[t] += hit & (l ^ 1);
    }
  }
  labelled = wave_reduce_add(labelled);
#pragma unroll
  for (int t = 0; t < SG_MAX_THRESHOLDS; ++t) {
    const int tp = wave_reduce_add(with[t]), fp = wave_reduce_add(without[t]);
    if ((threadIdx.x & 63) == 0 && t < num_thresholds) {
      unsigned long long* c = counts + ((long long)k * num_thresholds + t) * 3;
      if (tp) atomicAdd(c + 0, (unsigned long long)tp);
      if (fp) atomicAdd(c + 1, (unsigned long long)fp);
      if (labelled - tp) atomicAdd(c + 2, (unsigned long long)(labelled - tp));   // fn: labelled cells below the threshold
    }
  }
}

}  // namespace seg_head
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::seg_head;

extern "C" {

int bevamd_seg_iou_counts(const float* pred, const void* label, int label_dtype, int samples, int classes, long long hw,
                          const float* thresholds, int num_thresholds, long long* counts, void* stream) {
  // a thread counts in 32 bits: with at most 1024 classes a class has two workgroups or more, at most 2^27 cells per thread
  BEVAMD_REQUIRE(samples >= 1 && classes >= 1 && classes <= 1024 && hw >= 1 && samples <= (1LL << 36) / hw,
                 "seg_iou_counts: bad sizes (samples %d, classes %d (1 .. 1024), hw %lld; samples * hw up to 2^36)", samples, classes, hw);
  BEVAMD_REQUIRE(num_thresholds >= 1 && num_thresholds <= SG_MAX_THRESHOLDS, "seg_iou_counts: %d thresholds (1 .. %d)", num_thresholds,
                 SG_MAX_THRESHOLDS);
  BEVAMD_REQUIRE(pred && label && thresholds && counts, "seg_iou_counts: null pointer");
  if (label_dtype != 0 && label_dtype != 3) {
    set_error("seg_iou_counts: label_dtype %d (0 fp32, 3 uint8)", label_dtype);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const int n = classes * num_thresholds * 3;
  hipLaunchKernelGGL(iou_zero_kernel, dim3(cdiv(n, SG_THREADS)), dim3(SG_THREADS), 0, s, (unsigned long long*)counts, n);
  BEVAMD_LAUNCH_CHECK("seg_iou_counts zero");
  const long long per_class = hw * samples, per_block = (long long)SG_THREADS * SG_CELLS_PER_THREAD;
  long long blocks = (per_class + per_block - 1) / per_block;
  const long long cap = SG_MAX_GRID / classes;           // >= 2
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks, classes), block(SG_THREADS);
  if (label_dtype == 0)
    hipLaunchKernelGGL((iou_count_kernel<float>), grid, block, 0, s, pred, (const float*)label, samples, classes, hw, thresholds,
                       num_thresholds, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL((iou_count_kernel<unsigned char>), grid, block, 0, s, pred, (const unsigned char*)label, samples, classes, hw,
                       thresholds, num_thresholds, (unsigned long long*)counts);
  BEVAMD_LAUNCH_CHECK("seg_iou_counts");
  return BEVAMD_OK;
}

}  // extern "C"
