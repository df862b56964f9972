// TransFusion head training targets, gfx950: match costs, batched linear sum assignment, targets from the assignment.
//
// Replaces (reference):
//   mmdet3d/core/bbox/assigners/hungarian_assigner.py:13-35, 82-142   BBoxBEVL1Cost, IoU3DCost, HungarianAssigner3D.assign: per sample
//                                                      and decoder layer about 40 small torch ops, cost.detach().cpu(), scipy's
//                                                      linear_sum_assignment on the host, and two copies back
//   mmdet 2.x core/bbox/match_costs/match_cost.py      FocalLossCost, ClassificationCost (restated: mmdet is not vendored)
//   mmdet3d/core/bbox/structures/base_box3d.py:378-445 height_overlaps, overlaps (the IoU of BboxOverlaps3D on LiDAR boxes)
//   mmdet3d/models/heads/bbox/transfusion.py:424-524, 575   the rows of get_targets_single that follow from the assignment
//
// Native formulation, for all samples and layers at once (problem n = sample * layers + layer):
//   * sizes_kernel    one thread per problem: the live ground-truth count (0 for a sample over the bound) and a clean status word;
//   * cost_kernel     one thread per (problem, proposal, ground-truth slot below the bound): the three weighted costs in the
//                     reference's fp32 operation order, sigmoid / log / pow / exp evaluated in double and rounded once, the rotated
//                     BEV overlap by csrc/iou3d_box.h; slots past the live count are written as zeros;
//   * lsa_kernel      ONE WAVE per problem: shortest augmenting paths with dual variables (the Jonker-Volgenant form as Crouse
//                     states it, which is what scipy runs), over the smaller side, duals and path costs in fp64.  Columns are dealt
//                     to lanes (column j: lane j % 64); a column's state (shortest path cost, dual, predecessor, visited flag,
//                     matched row) lives in LDS and is touched by its owner lane only, so the inner loop has no barrier; the
//                     per-step argmin is six xor-shuffle stages on (cost, column).  Why one wave: the algorithm is a chain of
//                     dependent argmins (58 / 319 / 579 of them at 200 x 40 / 120 / 260); a step scans at most 16 columns per lane,
//                     so a second wave would add a barrier and an LDS exchange per step to split a scan that is already shorter
//                     than the reduction behind it.  The cost block is staged in LDS (in the solver's orientation, so that a scan
//                     reads consecutive words) when it fits beside the state, otherwise read from global memory through L2;
//   * targets_kernel  one workgroup: every row of labels / label_weights / bbox_targets / bbox_weights / ious, then num_pos and
//                     matched_ious by a fixed-order LDS reduction.
// No workspace, nothing read back, no atomics on float data: results are bit-equal from run to run.  Every output element is
// written on every call.  The unit is compiled with fp contract(off), and so is iou3d_box.h by the pragma in each of its
// functions (as in csrc/iou3d.hip); hipcc keeps fp32 divide correctly rounded.
//
// The solver cannot hang: one augmentation visits at most `cols` columns (a for loop over that bound), there are `rows`
// augmentations, and the path walk back from the sink is a for loop over `rows + 1` steps; a problem that would need more ends with
// status bit 8 and all rows unmatched.  Non-finite entries are rejected before the first augmentation.
#include "common.h"
#include "iou3d_box.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace bevamd {
namespace head_assign {

constexpr int HA_MAX_SIDE = 1024;      // rows, columns of one assignment problem; boxes per sample
constexpr int HA_MAX_CLASSES = 64;
constexpr int HA_THREADS = 256;
constexpr int HA_TARGET_THREADS = 1024;
constexpr int LSA_WAVE = 64;
constexpr size_t LSA_LDS_LIMIT = 64 * 1024;

// status bits (mirrored in include/bevfusion_amd_ext.h and head_assign.py)
constexpr int ST_NONFINITE = 1;   // a live cost entry is not finite
constexpr int ST_LABEL = 2;       // a ground-truth label outside [0, classes)
constexpr int ST_OVERFLOW = 4;    // the sample has more boxes than the bound, or its offsets name no range of the arrays
constexpr int ST_BOUND = 8;       // the solver's structural loop bound was reached, or a live size is outside the buffer

struct CostCfg {
  int batch, layers, k, gmax, classes, box_dim, num_rows;
  int cls_mode;                   // 0: none, 1: FocalLossCost, 2: ClassificationCost
  int use_reg, use_iou;
  float w_cls, w_reg, w_iou;
  float one_minus_alpha, alpha, eps;
  double gamma;
  float pc0, pc1, range0, range1; // point_cloud_range[0:2] and [3:5] - [0:2], each rounded to fp32 first
};

__device__ __forceinline__ float ha_round(double v) { return (float)v; }

// [first, first + count) of sample b; count 0 with over set as in head_targets.hip
__device__ __forceinline__ void ha_range(const int* __restrict__ offsets, int b, int bound, int num_rows, int& first, int& count,
                                         bool& over) {
  first = offsets[b];
  const long long n = (long long)offsets[b + 1] - first;
  over = n > bound || n < 0 || first < 0 || (long long)first + n > num_rows;
  count = over ? 0 : (int)n;
}

// ---- live sizes -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HA_THREADS) void sizes_kernel(const int* __restrict__ offsets, int batch, int layers, int bound,
                                                           int num_rows, int* __restrict__ num_gt, int* __restrict__ status) {
  const int n = blockIdx.x * HA_THREADS + threadIdx.x;
  if (n >= batch * layers) return;
  int first, count;
  bool over;
  ha_range(offsets, n / layers, bound, num_rows, first, count, over);
  num_gt[n] = count;
  status[n] = over ? ST_OVERFLOW : 0;
}

// ---- match costs ----------------------------------------------------------------------------------------------------------------
// x^gamma as torch evaluates pow on an fp32 tensor: the square is a multiply, everything else goes through double
__device__ __forceinline__ float ha_pow(float x, double gamma) {
  if (gamma == 2.0) return x * x;
  if (gamma == 1.0) return x;
  return ha_round(pow((double)x, gamma));
}

__device__ __forceinline__ float ha_cls_cost(const float* __restrict__ logits, int classes, int pitch, int label, const CostCfg& c) {
  // logits: this proposal's column of [C, P] (element stride pitch)
  if (c.cls_mode == 1) {
    const float p = ha_round(1.0 / (1.0 + exp(-(double)logits[(size_t)label * pitch])));
    const float neg = -ha_round(log((double)(1.f - p + c.eps))) * c.one_minus_alpha * ha_pow(p, c.gamma);
    const float pos = -ha_round(log((double)(p + c.eps))) * c.alpha * ha_pow(1.f - p, c.gamma);
    return (pos - neg) * c.w_cls;
  }
  double mx = -DBL_MAX;
  for (int q = 0; q < classes; ++q) mx = fmax(mx, (double)logits[(size_t)q * pitch]);
  double sum = 0.0;
  for (int q = 0; q < classes; ++q) sum += exp((double)logits[(size_t)q * pitch] - mx);
  const float s = ha_round(exp((double)logits[(size_t)label * pitch] - mx) / sum);
  return -s * c.w_cls;
}

// BaseInstance3DBoxes.overlaps for two LiDAR boxes (x, y, z bottom, dx, dy, dz, yaw)
__device__ __forceinline__ float ha_iou3d(const float* __restrict__ a, const float* __restrict__ b) {
  float xa[5] = {a[0] - a[3] / 2.f, a[1] - a[4] / 2.f, a[0] + a[3] / 2.f, a[1] + a[4] / 2.f, a[6]};
  float xb[5] = {b[0] - b[3] / 2.f, b[1] - b[4] / 2.f, b[0] + b[3] / 2.f, b[1] + b[4] / 2.f, b[6]};
  const float bev = iou3d::overlap(iou3d::make_box(xa), iou3d::make_box(xb));
  const float top = fminf(a[2] + a[5], b[2] + b[5]), bottom = fmaxf(a[2], b[2]);
  const float h = fmaxf(top - bottom, 0.f);
  const float o = bev * h;
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  return o / fmaxf(va + vb - o, 1e-8f);
}

__global__ __launch_bounds__(HA_THREADS) void cost_kernel(const float* __restrict__ boxes, const float* __restrict__ logits,
                                                          const float* __restrict__ gt_boxes, const long long* __restrict__ gt_labels,
                                                          const int* __restrict__ offsets, CostCfg c, float* __restrict__ cost,
                                                          float* __restrict__ iou, int* __restrict__ status) {
  const int n = blockIdx.y;                                   // problem
  const int e = blockIdx.x * HA_THREADS + threadIdx.x;        // (proposal, slot)
  if (e >= c.k * c.gmax) return;
  const int b = n / c.layers, l = n - b * c.layers;
  const int k = e / c.gmax, g = e - k * c.gmax;
  int first, count;
  bool over;
  ha_range(offsets, b, c.gmax, c.num_rows, first, count, over);
  const size_t at = (size_t)n * c.k * c.gmax + e;
  if (g >= count) {
    cost[at] = 0.f;
    iou[at] = 0.f;
    return;
  }
  const int P = c.layers * c.k, p = l * c.k + k;
  const float* gt = gt_boxes + (size_t)(first + g) * c.box_dim;
  float total = 0.f, overlap = 0.f;
  int flag = 0;
  if (c.cls_mode != 0) {
    const long long label = gt_labels[first + g];
    if (label < 0 || label >= c.classes) {
      flag |= ST_LABEL;
      total = __int_as_float(0x7fc00000);                     // never reaches the solver: it rejects the problem as well
    } else {
      total = ha_cls_cost(logits + (size_t)b * c.classes * P + p, c.classes, P, (int)label, c);
    }
  }
  const float* box = boxes != nullptr ? boxes + ((size_t)b * P + p) * c.box_dim : nullptr;
  if (c.use_reg) {
    const float ax = (box[0] - c.pc0) / c.range0, ay = (box[1] - c.pc1) / c.range1;
    const float gx = (gt[0] - c.pc0) / c.range0, gy = (gt[1] - c.pc1) / c.range1;
    total = total + (fabsf(ax - gx) + fabsf(ay - gy)) * c.w_reg;
  }
  if (c.use_iou) {
    overlap = ha_iou3d(box, gt);
    total = total + (-overlap) * c.w_iou;
  }
  if (!isfinite(total)) flag |= ST_NONFINITE;
  cost[at] = total;
  iou[at] = overlap;
  if (flag) atomicOr(status + n, flag);
}

// ---- linear sum assignment ------------------------------------------------------------------------------------------------------
// (value, key) minimum over the wave, the same in every lane.  key = (matched ? 1 << 16 : 0) | column: among equal path costs an
// unmatched column wins (as in scipy), then the lower column.
__device__ __forceinline__ void lsa_wave_argmin(double& v, int& key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int ok = __shfl_xor(key, o, 64);
    if (ov < v || (ov == v && ok < key)) {
      v = ov;
      key = ok;
    }
  }
}

// Dynamic LDS: doubles u[side_r], v[side_c], shortest[side_c]; ints path[side_c], row4col[side_c], col4row[side_r], visited[side_c];
// then `stage_floats` floats of the cost block.  side_r = min(R, C), side_c = max(R, C).
__global__ __launch_bounds__(LSA_WAVE) void lsa_kernel(const float* __restrict__ cost, const int* __restrict__ rows,
                                                       const int* __restrict__ cols, int R, int C, int stage_floats,
                                                       int* __restrict__ col4row_out, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lsa_lds[];
  const int side_r = R < C ? R : C, side_c = R < C ? C : R;
  double* u = (double*)lsa_lds;
  double* v = u + side_r;
  double* shortest = v + side_c;
  int* path = (int*)(shortest + side_c);
  int* row4col = path + side_c;
  int* col4row = row4col + side_c;
  int* visited = col4row + side_r;
  float* stage = (float*)(visited + side_c);

  const int n = blockIdx.x, lane = threadIdx.x;
  const float* cm = cost + (size_t)n * R * C;
  int* out = col4row_out + (size_t)n * R;
  const int nr0 = rows != nullptr ? rows[n] : R, nc0 = cols != nullptr ? cols[n] : C;
  int st = 0;
  if (nr0 < 0 || nr0 > R || nc0 < 0 || nc0 > C) st = ST_BOUND;
  const bool transpose = st == 0 && nr0 > nc0;                 // the solver's rows are the smaller side
  const int nr = st ? 0 : (transpose ? nc0 : nr0), nc = st ? 0 : (transpose ? nr0 : nc0);
  const bool staged = (long long)nr * nc <= stage_floats;

  // non-finite entries end the problem here; the live block is staged in the solver's orientation on the way
  int bad = 0;
  const int live = nr0 * nc0;                                  // <= 1024 * 1024
  if (st == 0) {
    for (int e = lane; e < live; e += LSA_WAVE) {
      const int r = e / nc0, q = e - r * nc0;
      const float x = cm[(size_t)r * C + q];
      bad |= isfinite(x) ? 0 : 1;
      if (staged) stage[transpose ? q * nc + r : e] = x;
    }
    if (__any(bad)) st = ST_NONFINITE;
  }
  for (int i = lane; i < nr; i += LSA_WAVE) {
    u[i] = 0.0;
    col4row[i] = -1;
  }
  for (int j = lane; j < nc; j += LSA_WAVE) {
    v[j] = 0.0;
    row4col[j] = -1;
  }
  __syncthreads();

  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  const long long rs = transpose ? 1 : C, cs = transpose ? C : 1;     // element strides of the solver's (row, column) in `cm`
  for (int cur = 0; cur < nr && st == 0; ++cur) {
    for (int j = lane; j < nc; j += LSA_WAVE) {
      shortest[j] = INF;
      path[j] = -1;
      visited[j] = 0;
    }
    int i = cur, sink = -1;
    double min_val = 0.0;
    for (int step = 0; step < nc; ++step) {                    // one augmentation visits at most nc columns
      const double ui = u[i];                                  // written behind the barrier that ends the previous augmentation
      double best = INF;
      int key = 0x7fffffff, best_row = -1;
      for (int j = lane; j < nc; j += LSA_WAVE) {
        if (visited[j]) continue;
        const float x = staged ? stage[i * nc + j] : cm[i * rs + j * cs];
        const double r = min_val + (double)x - ui - v[j];
        double s = shortest[j];
        if (r < s) {
          s = r;
          shortest[j] = r;
          path[j] = i;
        }
        const int m = row4col[j];
        const int kj = (m >= 0 ? 1 << 16 : 0) | j;
        if (s < best || (s == best && kj < key)) {
          best = s;
          key = kj;
          best_row = m;
        }
      }
      lsa_wave_argmin(best, key);
      if (key == 0x7fffffff || !(best < INF)) break;           // no reachable column: cannot happen with finite entries
      const int j = key & 0xffff;
      min_val = best;
      const int m = __shfl(best_row, j & (LSA_WAVE - 1), 64);  // the owner lane's candidate is column j
      if ((j & (LSA_WAVE - 1)) == lane) visited[j] = 1;
      if (m < 0) {
        sink = j;
        break;
      }
      i = m;
    }
    if (sink < 0) {
      st = ST_BOUND;
      break;
    }
    // dual updates: a visited column j other than the sink is matched to the visited row row4col[j], one column per row
    for (int j = lane; j < nc; j += LSA_WAVE) {
      if (!visited[j]) continue;
      const double d = min_val - shortest[j];
      v[j] -= d;
      const int m = row4col[j];
      if (m >= 0) u[m] += d;
    }
    if (lane == 0) u[cur] += min_val;
    __syncthreads();
    if (lane == 0) {
      int j = sink, done = 0;
      for (int t = 0; t <= nr; ++t) {                          // the path holds at most nr rows
        const int r = path[j];
        if (r < 0) break;
        row4col[j] = r;
        const int next = col4row[r];
        col4row[r] = j;
        j = next;
        if (r == cur) {
          done = 1;
          break;
        }
        if (j < 0) break;
      }
      visited[0] = done;                                       // visited is reset at the top of the next augmentation
    }
    __syncthreads();
    if (!visited[0]) st = ST_BOUND;
    __syncthreads();
  }

  for (int r = lane; r < R; r += LSA_WAVE) {
    int m = -1;
    if (st == 0 && r < nr0) m = transpose ? row4col[r] : col4row[r];
    out[r] = m;
  }
  if (lane == 0) status[n] = st;
}

// ---- targets --------------------------------------------------------------------------------------------------------------------
struct TargetCfg {
  int batch, layers, k, gmax, box_dim, num_rows, num_classes, code_size;
  long long pos_weight;           // <= 0: 1
  float pc0, pc1, div0, div1;     // div = out_size_factor * voxel_size, the product formed in double by the caller, rounded here
};

__global__ __launch_bounds__(HA_TARGET_THREADS) void targets_kernel(
    const int* __restrict__ col4row, const float* __restrict__ iou, const int* __restrict__ status_cost,
    const int* __restrict__ status_lsa, const float* __restrict__ gt_boxes, const long long* __restrict__ gt_labels,
    const int* __restrict__ offsets, TargetCfg c, long long* __restrict__ labels, long long* __restrict__ label_weights,
    float* __restrict__ bbox_targets, float* __restrict__ bbox_weights, float* __restrict__ ious, int* __restrict__ flags,
    int* __restrict__ num_pos, float* __restrict__ matched_ious) {
  __shared__ double s_sum[HA_TARGET_THREADS];
  __shared__ int s_cnt[HA_TARGET_THREADS];
  const int tid = threadIdx.x;
  const int P = c.layers * c.k;
  int total_pos = 0;
  double mean_sum = 0.0;
  for (int b = 0; b < c.batch; ++b) {
    int first, count;
    bool over;
    ha_range(offsets, b, c.gmax, c.num_rows, first, count, over);
    int flag = over ? ST_OVERFLOW : 0;
    for (int l = 0; l < c.layers; ++l) flag |= (status_cost != nullptr ? status_cost[b * c.layers + l] : 0) | status_lsa[b * c.layers + l];
    if (tid == 0) flags[b] = flag;
    double sum = 0.0;
    int cnt = 0;
    for (int p = tid; p < P; p += HA_TARGET_THREADS) {
      const int l = p / c.k, k = p - l * c.k;
      const size_t row = (size_t)b * P + p;
      const int g = flag ? -1 : col4row[(size_t)(b * c.layers + l) * c.k + k];
      float t[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      long long label = c.num_classes, weight = 1;
      float w = 0.f, ov = 0.f;
      if (g >= 0 && g < count) {
        const float* box = gt_boxes + (size_t)(first + g) * c.box_dim;
        label = gt_labels[first + g];
        weight = c.pos_weight > 0 ? c.pos_weight : 1;
        w = 1.f;
        ov = iou[((size_t)(b * c.layers + l) * c.k + k) * c.gmax + g];
        ov = fminf(fmaxf(ov, 0.f), 1.f);
        t[0] = (box[0] - c.pc0) / c.div0;
        t[1] = (box[1] - c.pc1) / c.div1;
        t[2] = box[2] + box[5] * 0.5f;                         // bottom centre to gravity centre
        for (int d = 0; d < 3; ++d) t[3 + d] = ha_round(log((double)box[3 + d]));
        t[6] = ha_round(sin((double)box[6]));
        t[7] = ha_round(cos((double)box[6]));
        if (c.code_size == 10) {
          t[8] = box[7];
          t[9] = box[8];
        }
        sum += (double)ov;
        cnt += 1;
      }
      labels[row] = label;
      label_weights[row] = weight;
      ious[row] = ov;
      for (int d = 0; d < c.code_size; ++d) {
        bbox_targets[row * c.code_size + d] = t[d];
        bbox_weights[row * c.code_size + d] = w;
      }
    }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = HA_TARGET_THREADS / 2; o > 0; o >>= 1) {      // fixed order: the same bits on every run
      if (tid < o) {
        s_sum[tid] += s_sum[tid + o];
        s_cnt[tid] += s_cnt[tid + o];
      }
      __syncthreads();
    }
    const int npos = s_cnt[0];
    total_pos += npos;
    mean_sum += (double)ha_round(s_sum[0] / (double)(npos > 1 ? npos : 1));   // float(mean_iou) of the sample
    __syncthreads();
  }
  if (tid == 0) {
    *num_pos = total_pos;
    *matched_ious = ha_round(mean_sum / (double)c.batch);
  }
}

static int check_gt(const char* what, int num_rows, int box_dim, int batch, int max_boxes) {
  BEVAMD_REQUIRE(num_rows >= 0 && batch >= 1 && batch <= 65535, "%s: bad sizes (rows %d, batch %d)", what, num_rows, batch);
  BEVAMD_REQUIRE(box_dim == 7 || box_dim == 9, "%s: boxes have 7 or 9 columns, got %d", what, box_dim);
  if (max_boxes < 1 || max_boxes > HA_MAX_SIDE) {
    set_error("%s: max_boxes_per_sample %d (1 .. %d)", what, max_boxes, HA_MAX_SIDE);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  return BEVAMD_OK;
}

static size_t lsa_state_bytes(int R, int C) {
  const size_t r = R < C ? R : C, c = R < C ? C : R;
  return 8 * (r + 2 * c) + 4 * (3 * c + r);
}

}  // namespace head_assign
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::head_assign;

extern "C" {

int bevamd_match_costs(const float* boxes, const float* logits, const float* gt_boxes, const long long* gt_labels, const int* offsets,
                       int num_rows, int box_dim, int batch, int layers, int num_proposals, int classes, int max_boxes_per_sample,
                       int cls_mode, float cls_weight, double alpha, double gamma, float eps, int use_reg, float reg_weight,
                       int use_iou, float iou_weight, const float* pc_range, float* cost, float* iou, int* num_gt, int* status,
                       void* stream) {
  const int rc = check_gt("match_costs", num_rows, box_dim, batch, max_boxes_per_sample);
  if (rc != BEVAMD_OK) return rc;
  if (num_proposals < 1 || num_proposals > HA_MAX_SIDE) {
    set_error("match_costs: %d proposals per layer (1 .. %d)", num_proposals, HA_MAX_SIDE);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(layers >= 1 && (long long)batch * layers <= 65535, "match_costs: %d layers x %d samples (at most 65535 problems)", layers,
                 batch);
  BEVAMD_REQUIRE(cls_mode >= 0 && cls_mode <= 2, "match_costs: cls_mode %d (0 none, 1 focal, 2 softmax)", cls_mode);
  if (cls_mode != 0 && (classes < 1 || classes > HA_MAX_CLASSES)) {
    set_error("match_costs: %d classes (1 .. %d)", classes, HA_MAX_CLASSES);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(offsets && cost && iou && num_gt && status && (gt_boxes || num_rows == 0), "match_costs: null pointer");
  BEVAMD_REQUIRE(cls_mode == 0 || (logits && gt_labels), "match_costs: a classification cost needs logits and labels");
  BEVAMD_REQUIRE((!use_reg && !use_iou) || boxes, "match_costs: box costs need boxes");
  BEVAMD_REQUIRE(!use_reg || pc_range, "match_costs: BBoxBEVL1Cost needs point_cloud_range (HOST, 6 floats)");
  CostCfg c{};
  c.batch = batch;
  c.layers = layers;
  c.k = num_proposals;
  c.gmax = max_boxes_per_sample;
  c.classes = classes;
  c.box_dim = box_dim;
  c.num_rows = num_rows;
  c.cls_mode = cls_mode;
  c.use_reg = use_reg ? 1 : 0;
  c.use_iou = use_iou ? 1 : 0;
  c.w_cls = cls_weight;
  c.w_reg = reg_weight;
  c.w_iou = iou_weight;
  c.alpha = (float)alpha;
  c.one_minus_alpha = (float)(1.0 - alpha);
  c.eps = eps;
  c.gamma = gamma;
  if (pc_range) {
    c.pc0 = pc_range[0];
    c.pc1 = pc_range[1];
    c.range0 = pc_range[3] - pc_range[0];
    c.range1 = pc_range[4] - pc_range[1];
  }
  hipStream_t s = (hipStream_t)stream;
  const int problems = batch * layers;
  hipLaunchKernelGGL(sizes_kernel, dim3(cdiv(problems, HA_THREADS)), dim3(HA_THREADS), 0, s, offsets, batch, layers, max_boxes_per_sample,
                     num_rows, num_gt, status);
  BEVAMD_LAUNCH_CHECK("match_costs sizes");
  hipLaunchKernelGGL(cost_kernel, dim3(cdiv((long long)num_proposals * max_boxes_per_sample, HA_THREADS), problems), dim3(HA_THREADS), 0, s,
                     boxes, logits, gt_boxes, gt_labels, offsets, c, cost, iou, status);
  BEVAMD_LAUNCH_CHECK("match_costs cost");
  return BEVAMD_OK;
}

int bevamd_linear_sum_assignment(const float* cost, const int* rows, const int* cols, int num_problems, int max_rows, int max_cols,
                                 int* col4row, int* status, void* stream) {
  if (max_rows < 1 || max_cols < 1 || max_rows > HA_MAX_SIDE || max_cols > HA_MAX_SIDE) {
    set_error("linear_sum_assignment: %d x %d (1 .. %d each side)", max_rows, max_cols, HA_MAX_SIDE);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(num_problems >= 1 && num_problems <= 0x7fffff, "linear_sum_assignment: %d problems", num_problems);
  BEVAMD_REQUIRE(cost && col4row && status, "linear_sum_assignment: null pointer");
  // the block is staged when it fits beside the state in the 64 KiB a workgroup gets without asking
  const size_t state = (lsa_state_bytes(max_rows, max_cols) + 15) / 16 * 16;
  const size_t block = (size_t)max_rows * max_cols * 4;
  const size_t bytes = state + block <= LSA_LDS_LIMIT ? state + block : state;
  const int stage_floats = (int)((bytes - state) / 4);
  hipLaunchKernelGGL(lsa_kernel, dim3(num_problems), dim3(LSA_WAVE), bytes, (hipStream_t)stream, cost, rows, cols, max_rows, max_cols,
                     stage_floats, col4row, status);
  BEVAMD_LAUNCH_CHECK("linear_sum_assignment");
  return BEVAMD_OK;
}

int bevamd_transfusion_assign_targets(const int* col4row, const float* iou, const int* status_cost, const int* status_lsa,
                                      const float* gt_boxes, const long long* gt_labels, const int* offsets, int num_rows, int box_dim,
                                      int batch, int layers, int num_proposals, int max_boxes_per_sample, int num_classes, int code_size,
                                      long long pos_weight, const double* coder,
                                      long long* labels, long long* label_weights, float* bbox_targets, float* bbox_weights, float* ious,
                                      int* flags, int* num_pos, float* matched_ious, void* stream) {
  const int rc = check_gt("transfusion_assign_targets", num_rows, box_dim, batch, max_boxes_per_sample);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(layers >= 1 && num_proposals >= 1 && num_proposals <= HA_MAX_SIDE && (long long)batch * layers <= 65535,
                 "transfusion_assign_targets: bad sizes (%d layers of %d proposals)", layers, num_proposals);
  BEVAMD_REQUIRE(code_size == 8 || (code_size == 10 && box_dim == 9), "transfusion_assign_targets: code_size %d with %d box columns (8, or 10 with 9)",
                 code_size, box_dim);
  BEVAMD_REQUIRE(num_classes >= 1 && coder, "transfusion_assign_targets: num_classes >= 1, coder a HOST array of 4 doubles");
  BEVAMD_REQUIRE(col4row && iou && status_lsa && gt_labels && offsets && labels && label_weights && bbox_targets && bbox_weights && ious &&
                     flags && num_pos && matched_ious && (gt_boxes || num_rows == 0),
                 "transfusion_assign_targets: null pointer");
  TargetCfg c{};
  c.batch = batch;
  c.layers = layers;
  c.k = num_proposals;
  c.gmax = max_boxes_per_sample;
  c.box_dim = box_dim;
  c.num_rows = num_rows;
  c.num_classes = num_classes;
  c.code_size = code_size;
  c.pos_weight = pos_weight;
  c.pc0 = (float)coder[0];
  c.pc1 = (float)coder[1];
  c.div0 = (float)coder[2];
  c.div1 = (float)coder[3];
  hipLaunchKernelGGL(targets_kernel, dim3(1), dim3(HA_TARGET_THREADS), 0, (hipStream_t)stream, col4row, iou, status_cost, status_lsa, gt_boxes,
                     gt_labels, offsets, c, labels, label_weights, bbox_targets, bbox_weights, ious, flags, num_pos, matched_ious);
  BEVAMD_LAUNCH_CHECK("transfusion_assign_targets");
  return BEVAMD_OK;
}

}  // extern "C"
