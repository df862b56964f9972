// Training targets of the two detection heads, gfx950: Gaussian heatmaps and the CenterHead box / index / mask rows.
//
// Replaces (reference):
//   mmdet3d/models/heads/bbox/centerpoint.py:432-582   CenterHead.get_targets_single: a Python loop over tasks x boxes of about 30
//                                                      zero-dimensional torch ops each, three of them host read-backs, and a numpy
//                                                      Gaussian copied to the device per box
//   mmdet3d/models/heads/bbox/transfusion.py:526-573   the dense heatmap of TransFusionHead.get_targets_single, the same loop
//   mmdet3d/core/utils/gaussian.py                     gaussian_radius, gaussian_2d, draw_heatmap_gaussian
//
// Native formulation, packed inputs (boxes [M, 7|9], labels [M] int64, offsets [B + 1] int32 on the device):
//   * zero_kernel        the heatmap is zeroed inside the call: a replay starts clean;
//   * slots_kernel       (CenterHead) one workgroup per sample ranks its boxes class-major, stable within a class, in LDS and
//                        writes EVERY (task, slot) row of anno_box / ind / mask once, with values or with zeros;
//   * draw_kernel        one workgroup per (sample, box position below the caller's bound) recomputes the box's cell and radius
//                        with the device function the slots use and walks its clipped window: the value is evaluated in double,
//                        rounded once to fp32 and combined with an unsigned atomicMax on the bit pattern (all values lie in (0, 1],
//                        where the bit pattern orders like the value), so the result does not depend on the order of arrival.
// bevamd_centerhead_targets: 3 launches; bevamd_heatmap_targets: 2 launches; for any B, M and box contents.  No workspace, nothing
// read back.  The unit is compiled with fp contract(off): the radius and the cell round like the reference's separate CPU fp32
// multiplies, divides and square roots (hipcc keeps fp32 divide and square root correctly rounded unless asked otherwise, and the
// build does not ask); log / sin / cos / exp are evaluated in double and rounded once.
#include "common.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace bevamd {
namespace head_targets {

constexpr int HT_MAX_BOXES = 1024;   // boxes per sample (the caller's bound may be lower)
constexpr int HT_MAX_TASKS = 16;
constexpr int HT_MAX_CLASSES = 64;
constexpr int HT_THREADS = 256;

struct HtCfg {
  int num_tasks;                 // 0: the TransFusion flavour (no tasks, plane = label)
  int flag[HT_MAX_TASKS + 1];    // task t owns the labels [flag[t], flag[t + 1])
  int total_classes;
  int batch, size;               // square maps: size x size
  int max_objs, max_boxes, num_rows, box_dim;
  int min_radius, norm_bbox;
  float pc0, pc1, vs0, vs1, osf;
  // gaussian_radius's Python-float constants, formed in double and rounded where they meet the fp32 tensor
  float one_minus, one_plus, minus_two_m, m_minus_one, sixteen_m;
};

struct HtGeo {
  float coor_x, coor_y;
  int cell_x, cell_y, radius;
};

// gaussian.py:55-84 on fp32 scalars as CPU torch evaluates it (height = length, width = width).
__device__ __forceinline__ float ht_gaussian_radius(float height, float width, const HtCfg& c) {
  const float hw = height + width;
  const float b1 = hw;
  const float c1 = width * height * c.one_minus / c.one_plus;
  const float r1 = (b1 + sqrtf(b1 * b1 - 4.f * c1)) / 2.f;
  const float b2 = 2.f * hw;
  const float c2 = c.one_minus * width * height;
  const float r2 = (b2 + sqrtf(b2 * b2 - 16.f * c2)) / 2.f;
  const float b3 = c.minus_two_m * hw;
  const float c3 = c.m_minus_one * width * height;
  const float r3 = (b3 + sqrtf(b3 * b3 - c.sixteen_m * c3)) / 2.f;
  float r = r1;                       // Python's min(r1, r2, r3): the first of the smallest
  if (r2 < r) r = r2;
  if (r3 < r) r = r3;
  return r;
}

// The size test, the radius and the centre cell of one box (centerpoint.py:505-546, transfusion.py:541-566); false: skipped.
__device__ __forceinline__ bool ht_geometry(const float* __restrict__ box, const HtCfg& c, HtGeo& g) {
  const float width = box[3] / c.vs0 / c.osf;
  const float length = box[4] / c.vs1 / c.osf;
  if (!(width > 0.f && length > 0.f)) return false;
  const float r = ht_gaussian_radius(length, width, c);
  int ri = r < 1073741824.f ? (int)r : 1073741824;   // int(radius) truncates; a window is clipped to the map anyway
  g.radius = ri > c.min_radius ? ri : c.min_radius;
  g.coor_x = (box[0] - c.pc0) / c.vs0 / c.osf;
  g.coor_y = (box[1] - c.pc1) / c.vs1 / c.osf;
  // .to(torch.int32) truncates toward zero: the cell lies in [0, size) exactly when the coordinate lies in (-1, size)
  const float s = (float)c.size;
  if (!(g.coor_x > -1.f && g.coor_x < s && g.coor_y > -1.f && g.coor_y < s)) return false;
  g.cell_x = (int)g.coor_x;
  g.cell_y = (int)g.coor_y;
  return true;
}

// [first, first + count) of sample b in the packed arrays; count 0 with *over set when the sample exceeds the bound (or the
// offsets do not describe a range of the arrays: nothing outside them is ever read).
__device__ __forceinline__ void ht_range(const int* __restrict__ offsets, int b, const HtCfg& c, int& first, int& count, bool& over) {
  first = offsets[b];
  const long long n = (long long)offsets[b + 1] - first;
  over = n > c.max_boxes || n < 0 || first < 0 || (long long)first + n > c.num_rows;
  count = over ? 0 : (int)n;
}

__device__ __forceinline__ int ht_task_of(int label, const HtCfg& c) {
  for (int t = 0; t < c.num_tasks; ++t)
    if (label < c.flag[t + 1]) return t;
  return c.num_tasks - 1;
}

__device__ __forceinline__ float ht_round(double v) { return (float)v; }

// ---- zero ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HT_THREADS) void zero_kernel(unsigned* __restrict__ p, size_t n) {
  const size_t stride = (size_t)gridDim.x * HT_THREADS;
  for (size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

// ---- CenterHead slots ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HT_THREADS) void slots_kernel(const float* __restrict__ boxes, const long long* __restrict__ labels,
                                                           const int* __restrict__ offsets, HtCfg c, float* __restrict__ anno_box,
                                                           long long* __restrict__ ind, unsigned char* __restrict__ mask,
                                                           int* __restrict__ overflow) {
  __shared__ int s_label[HT_MAX_BOXES];              // -1: owned by no task
  __shared__ unsigned short s_order[HT_MAX_BOXES];   // box at every class-major position
  __shared__ int s_start[HT_MAX_TASKS + 1];          // first position of every task
  const int b = blockIdx.x, tid = threadIdx.x;
  int first, n;
  bool over;
  ht_range(offsets, b, c, first, n, over);
  if (tid == 0) overflow[b] = over ? 1 : 0;
  for (int i = tid; i < n; i += HT_THREADS) {
    const long long l = labels[first + i];
    s_label[i] = (l >= 0 && l < c.total_classes) ? (int)l : -1;
  }
  __syncthreads();
  for (int i = tid; i < n; i += HT_THREADS) {
    const int l = s_label[i];
    if (l < 0) continue;
    int p = 0;
    for (int j = 0; j < n; ++j) {
      const int lj = s_label[j];
      p += (lj >= 0 && (lj < l || (lj == l && j < i))) ? 1 : 0;
    }
    s_order[p] = (unsigned short)i;                  // p < n <= HT_MAX_BOXES: positions of owned boxes are distinct
  }
  if (tid <= c.num_tasks) {
    int p = 0;
    for (int j = 0; j < n; ++j) p += (s_label[j] >= 0 && s_label[j] < c.flag[tid]) ? 1 : 0;
    s_start[tid] = p;
  }
  __syncthreads();
  const int slots = c.num_tasks * c.max_objs;
  for (int s = tid; s < slots; s += HT_THREADS) {
    const int t = s / c.max_objs, k = s - t * c.max_objs;
    const size_t at = ((size_t)t * c.batch + b) * c.max_objs + k;
    float row[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    long long cell = 0;
    unsigned char live = 0;
    if (k < s_start[t + 1] - s_start[t]) {
      const float* box = boxes + (size_t)(first + s_order[s_start[t] + k]) * c.box_dim;
      HtGeo g;
      if (ht_geometry(box, c, g)) {
        live = 1;
        cell = (long long)g.cell_x * c.size + g.cell_y;
        row[0] = g.coor_x - (float)g.cell_x;
        row[1] = g.coor_y - (float)g.cell_y;
        row[2] = box[2] + box[5] * 0.5f;             // the gravity centre (lidar_box3d.py:45)
        for (int d = 0; d < 3; ++d) row[3 + d] = c.norm_bbox ? ht_round(log((double)box[3 + d])) : box[3 + d];
        row[6] = ht_round(sin((double)box[6]));
        row[7] = ht_round(cos((double)box[6]));
        if (c.box_dim >= 9) {
          row[8] = box[7];
          row[9] = box[8];
        }
      }
    }
    for (int d = 0; d < 10; ++d) anno_box[at * 10 + d] = row[d];
    ind[at] = cell;
    mask[at] = live;
  }
}

// ---- draw ---------------------------------------------------------------------------------------------------------------------
// draw_heatmap_gaussian(heatmap[plane], center_int[[1, 0]], radius): row = cell_x, column = cell_y.
__global__ __launch_bounds__(HT_THREADS) void draw_kernel(const float* __restrict__ boxes, const long long* __restrict__ labels,
                                                          const int* __restrict__ offsets, HtCfg c, unsigned* __restrict__ heatmap,
                                                          int* __restrict__ overflow) {
  __shared__ int s_rank;
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int first, n;
  bool over;
  ht_range(offsets, b, c, first, n, over);
  if (overflow != nullptr && i == 0 && tid == 0) overflow[b] = over ? 1 : 0;
  if (i >= n) return;
  const long long l64 = labels[first + i];
  if (l64 < 0 || l64 >= c.total_classes) return;
  const int l = (int)l64;
  HtGeo g;
  if (!ht_geometry(boxes + (size_t)(first + i) * c.box_dim, c, g)) return;
  const size_t hw = (size_t)c.size * c.size;
  size_t plane;
  if (c.num_tasks > 0) {
    // only the first max_objs boxes of a task in class-major order are drawn
    const int t = ht_task_of(l, c);
    if (tid == 0) s_rank = 0;
    __syncthreads();
    int p = 0;
    for (int j = tid; j < n; j += HT_THREADS) {
      const long long lj = labels[first + j];
      p += (lj >= c.flag[t] && (lj < l || (lj == l && j < i))) ? 1 : 0;
    }
    if (p) atomicAdd(&s_rank, p);
    __syncthreads();
    if (s_rank >= c.max_objs) return;
    const int ct = c.flag[t + 1] - c.flag[t];
    plane = (size_t)c.batch * c.flag[t] + (size_t)b * ct + (l - c.flag[t]);   // each task's [B, C_t, H, W] block is contiguous
  } else {
    plane = (size_t)b * c.total_classes + l;
  }
  const int size = c.size, r = g.radius;
  const int x = g.cell_y, y = g.cell_x;
  const int left = min(x, r), right = min(size - x, r + 1), top = min(y, r), bottom = min(size - y, r + 1);
  const int w = left + right, cells = w * (top + bottom);                     // <= size * size
  const double sigma = (2.0 * r + 1.0) / 6.0;
  const double denom = 2.0 * sigma * sigma;
  unsigned* out = heatmap + plane * hw + (size_t)(y - top) * size + (x - left);
  for (int q = tid; q < cells; q += HT_THREADS) {
    const int wy = q / w, wx = q - wy * w;
    const double dy = (double)(wy - top), dx = (double)(wx - left);
    const double v = exp(-(dx * dx + dy * dy) / denom);
    if (v < DBL_EPSILON) continue;                                             // h[h < eps * h.max()] = 0, h.max() = 1
    atomicMax(out + (size_t)wy * size + wx, __float_as_uint(ht_round(v)));
  }
}

static int fill_cfg(HtCfg& c, const char* what, int num_rows, int box_dim, int batch, int max_boxes, const int* task_classes,
                    int num_tasks, int classes, int max_objs, const float* pc_range, const float* voxel_size, int out_size_factor,
                    int size, double overlap, int min_radius, int norm_bbox) {
  BEVAMD_REQUIRE(num_rows >= 0 && batch >= 1 && batch <= 65535 && size >= 1 && size <= 32768 && out_size_factor >= 1 && min_radius >= 0,
                 "%s: bad sizes (rows %d, batch %d, map %d, out_size_factor %d, min_radius %d)", what, num_rows, batch, size,
                 out_size_factor, min_radius);
  BEVAMD_REQUIRE(box_dim == 7 || box_dim == 9, "%s: boxes have 7 or 9 columns, got %d", what, box_dim);
  BEVAMD_REQUIRE(pc_range != nullptr && voxel_size != nullptr, "%s: pc_range and voxel_size are host arrays of 2 floats", what);
  if (max_boxes < 1 || max_boxes > HT_MAX_BOXES) {
    set_error("%s: max_boxes_per_sample %d (1 .. %d)", what, max_boxes, HT_MAX_BOXES);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  c = HtCfg{};
  c.num_tasks = num_tasks;
  int total = classes;
  if (num_tasks > 0) {
    BEVAMD_REQUIRE(task_classes != nullptr && num_tasks <= HT_MAX_TASKS && max_objs >= 1, "%s: 1 .. %d tasks as a host table, max_objs >= 1",
                   what, HT_MAX_TASKS);
    total = 0;
    for (int t = 0; t < num_tasks; ++t) {
      BEVAMD_REQUIRE(task_classes[t] >= 1, "%s: task %d has %d classes", what, t, task_classes[t]);
      c.flag[t] = total;
      total += task_classes[t];
    }
    c.flag[num_tasks] = total;
  }
  if (total < 1 || total > HT_MAX_CLASSES) {
    set_error("%s: %d classes (1 .. %d)", what, total, HT_MAX_CLASSES);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  c.total_classes = total;
  c.batch = batch;
  c.size = size;
  c.max_objs = max_objs;
  c.max_boxes = max_boxes;
  c.num_rows = num_rows;
  c.box_dim = box_dim;
  c.min_radius = min_radius;
  c.norm_bbox = norm_bbox;
  c.pc0 = pc_range[0];
  c.pc1 = pc_range[1];
  c.vs0 = voxel_size[0];
  c.vs1 = voxel_size[1];
  c.osf = (float)out_size_factor;
  c.one_minus = (float)(1.0 - overlap);
  c.one_plus = (float)(1.0 + overlap);
  c.minus_two_m = (float)(-2.0 * overlap);
  c.m_minus_one = (float)(overlap - 1.0);
  c.sixteen_m = (float)(4.0 * (4.0 * overlap));
  return BEVAMD_OK;
}

static int zero_words(void* p, size_t words, hipStream_t stream) {
  const int grid = (int)(words / HT_THREADS < 4096 ? words / HT_THREADS + 1 : 4096);
  hipLaunchKernelGGL(zero_kernel, dim3(grid), dim3(HT_THREADS), 0, stream, (unsigned*)p, words);
  BEVAMD_LAUNCH_CHECK("head_targets zero");
  return BEVAMD_OK;
}

}  // namespace head_targets
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::head_targets;

extern "C" {

int bevamd_centerhead_targets(const float* boxes, const long long* labels, const int* offsets, int num_rows, int box_dim, int batch,
                              int max_boxes_per_sample, const int* task_classes, int num_tasks, int max_objs, const float* pc_range,
                              const float* voxel_size, int out_size_factor, int map_size, double gaussian_overlap, int min_radius,
                              int norm_bbox, float* heatmap, float* anno_box, long long* ind, unsigned char* mask, int* overflow,
                              void* stream) {
  HtCfg c;
  BEVAMD_REQUIRE(num_tasks >= 1, "centerhead_targets: %d tasks", num_tasks);
  const int rc = fill_cfg(c, "centerhead_targets", num_rows, box_dim, batch, max_boxes_per_sample, task_classes, num_tasks, 0, max_objs,
                          pc_range, voxel_size, out_size_factor, map_size, gaussian_overlap, min_radius, norm_bbox);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE((long long)num_tasks * max_objs <= 0x7fffffffLL, "centerhead_targets: %d tasks x %d slots", num_tasks, max_objs);
  BEVAMD_REQUIRE(labels && offsets && heatmap && anno_box && ind && mask && overflow && (boxes || num_rows == 0),
                 "centerhead_targets: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int z = zero_words(heatmap, (size_t)batch * c.total_classes * map_size * map_size, s);
  if (z != BEVAMD_OK) return z;
  hipLaunchKernelGGL(slots_kernel, dim3(batch), dim3(HT_THREADS), 0, s, boxes, labels, offsets, c, anno_box, ind, mask, overflow);
  BEVAMD_LAUNCH_CHECK("centerhead_targets slots");
  hipLaunchKernelGGL(draw_kernel, dim3(max_boxes_per_sample, batch), dim3(HT_THREADS), 0, s, boxes, labels, offsets, c,
                     (unsigned*)heatmap, (int*)nullptr);
  BEVAMD_LAUNCH_CHECK("centerhead_targets draw");
  return BEVAMD_OK;
}

int bevamd_heatmap_targets(const float* boxes, const long long* labels, const int* offsets, int num_rows, int box_dim, int batch,
                           int max_boxes_per_sample, int num_classes, const float* pc_range, const float* voxel_size,
                           int out_size_factor, int map_size, double gaussian_overlap, int min_radius, float* heatmap, int* overflow,
                           void* stream) {
  HtCfg c;
  const int rc = fill_cfg(c, "heatmap_targets", num_rows, box_dim, batch, max_boxes_per_sample, nullptr, 0, num_classes, 0, pc_range,
                          voxel_size, out_size_factor, map_size, gaussian_overlap, min_radius, 0);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(labels && offsets && heatmap && overflow && (boxes || num_rows == 0), "heatmap_targets: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int z = zero_words(heatmap, (size_t)batch * c.total_classes * map_size * map_size, s);
  if (z != BEVAMD_OK) return z;
  hipLaunchKernelGGL(draw_kernel, dim3(max_boxes_per_sample, batch), dim3(HT_THREADS), 0, s, boxes, labels, offsets, c,
                     (unsigned*)heatmap, overflow);
  BEVAMD_LAUNCH_CHECK("heatmap_targets draw");
  return BEVAMD_OK;
}

}  // extern "C"
