// The non-learned end of CenterHead (CenterPoint), gfx950.
//
// Replaces (reference):
//   mmdet3d/models/heads/bbox/centerpoint.py:637-757   get_bboxes: per task a sigmoid and an exp over whole maps, the coder's
//                                                      decode, then per sample a numba circle NMS behind .cpu().numpy() or nms_gpu
//   centerpoint.py:759-884                             get_task_detections: boolean-mask indexing (a host sync each), nms_gpu
//   core/bbox/coders/centerpoint_bbox_coders.py:62-225 two torch.topk calls and five permute().contiguous() copies of whole
//                                                      regression maps to gather K rows of each
//   ops/iou3d/src/iou3d.cpp:96-133                     the suppression mask copied to the host and swept there
//
// Native formulation, every task and sample in ONE launch each; the segment is (sample, task), s = sample * T + task:
//   * keys: sigmoid of every cell as a 64-bit key (order-preserving score bits high, complemented flat index c * H * W + cell low);
//   * select: he_select_segment (head_select.h) per segment.  The reference's two-level top-K (per class, then over classes * K)
//     equals the global top-K of the segment, and key order is its defined order;
//   * gather-decode: one thread per selected row reads reg / height / dim / rot / vel at its cell straight from the [B, c, H, W]
//     maps, in the reference's fp32 operation order, and writes the box, the merged label and the two masks;
//   * segmented rotated NMS: one workgroup per segment.  Live rows (already in descending score) are compacted into LDS as BEV
//     boxes; per block of 64 rows all waves share the block's 64 x 63 / 2 pairs, wave `block` resolves the block greedily on a
//     64-bit word, and every later live row tests itself against the rows the block kept.  No K x K mask, nothing leaves the device.
// Circle tasks go through bevamd_circle_nms (head_ends.hip).
// The rotated-overlap arithmetic is iou3d.hip's (iou3d_box.h), which carries fp contract(off) in its own functions, so both units
// evaluate it alike; everything after the pragma below is compiled with fp contract(off) too: products and sums round separately
// like the reference's separate torch ops.  exp and atan2 are evaluated in double and rounded once.
#include "common.h"
#include "iou3d_box.h"
#include "head_select.h"

#include <math.h>

#pragma clang fp contract(off)

namespace bevamd {
namespace head {

constexpr int CP_MAX_TASKS = 16;
constexpr int CP_MAX_CLASSES = 8;   // per task

struct CpTasks {
  int T;
  int total_classes;
  int classes[CP_MAX_TASKS];
  int class_base[CP_MAX_TASKS];   // classes of the tasks before this one: the label offset and the key offset / (H * W)
  const float* heat[CP_MAX_TASKS];
};

struct CpMaps {
  const float* reg[CP_MAX_TASKS];
  const float* hei[CP_MAX_TASKS];
  const float* dim[CP_MAX_TASKS];
  const float* rot[CP_MAX_TASKS];
  const float* vel[CP_MAX_TASKS];
  int rotate[CP_MAX_TASKS];   // 1: the task's rows meet the head's score test before its rotated NMS
};

struct CpConst {
  float osf, vs0, vs1, pc0, pc1;
  float clo[3], chi[3];   // the coder's post_center_range
  float plo[3], phi[3];   // the head's post_center_limit_range
  int has_post;
  float cthr, hthr;
  int use_cthr, use_hthr, norm_bbox, bottom_centre, has_reg, has_vel;
};

struct CpNms {
  int T;
  int enabled[CP_MAX_TASKS];
  int label_base[CP_MAX_TASKS];
  float thr[CP_MAX_TASKS];
  float scale[CP_MAX_TASKS][CP_MAX_CLASSES];
};

__device__ __forceinline__ unsigned cp_order_bits(float v) {   // unsigned order = float order
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cp_score_of(unsigned long long key) {
  const unsigned b = (unsigned)(key >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

// ---- (a) keys, (b) select -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cp_keys_kernel(CpTasks tt, unsigned hw, int apply_sigmoid, unsigned long long* __restrict__ cand) {
  const int s = blockIdx.y, b = s / tt.T, t = s - b * tt.T;
  const unsigned chw = (unsigned)tt.classes[t] * hw;
  const unsigned flat = blockIdx.x * 256u + threadIdx.x;
  if (flat >= chw) return;
  const float v = tt.heat[t][(size_t)b * chw + flat];
  const float sc = apply_sigmoid ? he_sigmoid(v) : v;
  cand[((size_t)b * tt.total_classes + tt.class_base[t]) * hw + flat] =
      ((unsigned long long)cp_order_bits(sc) << 32) | (unsigned long long)(~flat);
}

__global__ __launch_bounds__(HE_SEL_THREADS) void cp_select_kernel(CpTasks tt, unsigned hw, int K,
                                                                   const unsigned long long* __restrict__ cand,
                                                                   int* __restrict__ top_flat, float* __restrict__ top_score) {
  const int s = blockIdx.x, b = s / tt.T, t = s - b * tt.T;
  const unsigned chw = (unsigned)tt.classes[t] * hw;
  const size_t out0 = (size_t)s * K;
  he_select_segment(cand + ((size_t)b * tt.total_classes + tt.class_base[t]) * hw, chw, chw, K,
                    [=](unsigned pos, unsigned long long key) {
                      top_flat[out0 + pos] = (int)(~(unsigned)key);
                      top_score[out0 + pos] = cp_score_of(key);
                    });
}

// ---- (c) gather-decode ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cp_decode_kernel(CpTasks tt, CpMaps mp, CpConst cc, int B, int H, int W, int K,
                                                        const int* __restrict__ top_flat, const float* __restrict__ top_score,
                                                        float* __restrict__ boxes, int* __restrict__ labels,
                                                        unsigned char* __restrict__ live, unsigned char* __restrict__ post_ok) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * tt.T * K) return;
  const int s = (int)(e / K), b = s / tt.T, t = s - b * tt.T;
  const unsigned hw = (unsigned)H * W;
  const int width = cc.has_vel ? 9 : 7;
  float* __restrict__ o = boxes + (size_t)e * width;
  const unsigned flat = (unsigned)top_flat[e];
  if (flat >= (unsigned)tt.classes[t] * hw) {   // not a cell of this task's map: reads nothing, a dead row of zeros
    for (int j = 0; j < width; ++j) o[j] = 0.f;
    labels[e] = tt.class_base[t];
    live[e] = 0;
    post_ok[e] = 0;
    return;
  }
  const unsigned c = flat / hw, cell = flat - c * hw;
  const float sc = top_score[e];
  // centerpoint_bbox_coders.py:87-90: the FIRST coordinate is the row (ind // W), the second the column
  float x = (float)(cell / (unsigned)W), y = (float)(cell % (unsigned)W);
  if (cc.has_reg) {
    x = x + mp.reg[t][((size_t)b * 2 + 0) * hw + cell];
    y = y + mp.reg[t][((size_t)b * 2 + 1) * hw + cell];
  } else {
    x = x + 0.5f;
    y = y + 0.5f;
  }
  x = x * cc.osf * cc.vs0 + cc.pc0;
  y = y * cc.osf * cc.vs1 + cc.pc1;
  const float z = mp.hei[t][(size_t)b * hw + cell];
  float d[3];
  for (int j = 0; j < 3; ++j) {
    const float v = mp.dim[t][((size_t)b * 3 + j) * hw + cell];
    d[j] = cc.norm_bbox ? (float)exp((double)v) : v;
  }
  const float yaw = (float)atan2((double)mp.rot[t][((size_t)b * 2 + 0) * hw + cell], (double)mp.rot[t][((size_t)b * 2 + 1) * hw + cell]);
  o[0] = x; o[1] = y;
  o[2] = cc.bottom_centre ? z - d[2] * 0.5f : z;   // centerpoint.py:746, gravity centre to bottom centre; the range tests see the centre
  o[3] = d[0]; o[4] = d[1]; o[5] = d[2]; o[6] = yaw;
  if (cc.has_vel) {
    o[7] = mp.vel[t][((size_t)b * 2 + 0) * hw + cell];
    o[8] = mp.vel[t][((size_t)b * 2 + 1) * hw + cell];
  }
  labels[e] = tt.class_base[t] + (int)c;
  bool ok = x >= cc.clo[0] && y >= cc.clo[1] && z >= cc.clo[2] && x <= cc.chi[0] && y <= cc.chi[1] && z <= cc.chi[2];
  if (cc.use_cthr) ok = ok && sc > cc.cthr;                           // the coder: >
  if (mp.rotate[t] && cc.use_hthr) ok = ok && sc >= cc.hthr;          // get_task_detections: >=
  live[e] = ok ? 1 : 0;
  bool post = true;
  if (mp.rotate[t] && cc.has_post)
    post = x >= cc.plo[0] && y >= cc.plo[1] && z >= cc.plo[2] && x <= cc.phi[0] && y <= cc.phi[1] && z <= cc.phi[2];
  post_ok[e] = post ? 1 : 0;
}

// ---- (d) segmented rotated NMS -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HE_MAX_K) void rotate_nms_kernel(const float* __restrict__ boxes, int width, const int* __restrict__ labels,
                                                              const unsigned char* __restrict__ live,
                                                              const unsigned char* __restrict__ post_ok, int R, int pre_max, int pms,
                                                              CpNms nt, unsigned char* __restrict__ keep, int* __restrict__ counts) {
  __shared__ float sb[5][HE_MAX_K];            // sorted position -> (x1, y1, x2, y2, yaw)
  __shared__ short sid[HE_MAX_K];              // sorted position -> row of the segment
  __shared__ unsigned char ssup[HE_MAX_K];     // sorted position -> suppressed by a kept row of an earlier block
  __shared__ unsigned char kflag[HE_MAX_K];    // row of the segment -> kept
  __shared__ unsigned long long diag[64];      // row of the current block -> earlier rows of the block that suppress it
  __shared__ unsigned long long kept_w[HE_MAX_K / 64];
  __shared__ unsigned s_wcnt[HE_MAX_K / 64];
  __shared__ int s_count;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, task = s % nt.T;
  const size_t row0 = (size_t)s * R;
  if (!nt.enabled[task]) {   // a segment of another NMS type
    if (tid < R) keep[row0 + tid] = 0;
    if (tid == 0) counts[s] = 0;
    return;
  }
  const float thr = nt.thr[task];

  // live rows, in row order (descending score), cut to pre_max
  const bool alive = tid < R && (!live || live[row0 + tid]);
  const unsigned long long bal = __ballot(alive);
  if (lane == 0) s_wcnt[wave] = (unsigned)__popcll(bal);
  kflag[tid] = 0;
  ssup[tid] = 0;
  if (tid < HE_MAX_K / 64) kept_w[tid] = 0;
  if (tid == 0) s_count = 0;
  __syncthreads();
  unsigned pos = (unsigned)__popcll(bal & lanemask_lt()), all = 0;
  for (int w = 0; w < HE_MAX_K / 64; ++w) {
    if (w < wave) pos += s_wcnt[w];
    all += s_wcnt[w];
  }
  const int m = (int)min(all, (unsigned)max(pre_max, 0));
  if (alive && (int)pos < m) {
    const float* __restrict__ bx = boxes + (row0 + tid) * width;
    int cls = labels ? labels[row0 + tid] - nt.label_base[task] : 0;
    cls = min(max(cls, 0), CP_MAX_CLASSES - 1);
    const float sc = nt.scale[task][cls];
    // box.bev = (x, y, w, l, yaw) with w, l scaled (centerpoint.py:829-832), then xywhr2xyxyr
    const float hw_ = bx[3] * sc / 2, hl = bx[4] * sc / 2;
    sb[0][pos] = bx[0] - hw_;
    sb[1][pos] = bx[1] - hl;
    sb[2][pos] = bx[0] + hw_;
    sb[3][pos] = bx[1] + hl;
    sb[4][pos] = bx[6];
    sid[pos] = (short)tid;
  }
  __syncthreads();

  auto box_at = [&](int q) {
    const float v[5] = {sb[0][q], sb[1][q], sb[2][q], sb[3][q], sb[4][q]};
    return iou3d::make_box(v);
  };

  int total = 0;
  bool sup = false;
  const int nblk = (m + 63) >> 6;
  for (int rb = 0; rb < nblk; ++rb) {
    const int base = rb * 64;
    if (tid < 64) diag[tid] = 0;
    __syncthreads();
    // the block's pairs (earlier j, later i = lane) over all waves: wave w takes j = 4 w .. 4 w + 3
    if (base + lane < m && !ssup[base + lane]) {
      unsigned long long bits = 0;
      bool have = false;
      iou3d::Box later;
      for (int j = 4 * wave; j < 4 * wave + 4 && j < lane; ++j) {
        if (ssup[base + j]) continue;
        if (!have) {
          later = box_at(base + lane);
          have = true;
        }
        const iou3d::Box earlier = box_at(base + j);
        if (iou3d::iou_rotated(earlier, later) > thr) bits |= 1ull << j;
      }
      if (bits) atomicOr(&diag[lane], bits);
    }
    __syncthreads();
    if (wave == rb) {
      const bool can = base + lane < m && !ssup[base + lane];
      const unsigned long long d = diag[lane];
      unsigned long long kept = 0;
      for (int t = 0; t < 64; ++t) {
        const int mine_kept = (can && (d & kept) == 0ull) ? 1 : 0;
        if (__shfl(mine_kept, t, 64)) kept |= 1ull << t;
      }
      if (lane == 0) kept_w[rb] = kept;
    }
    __syncthreads();
    unsigned long long k = kept_w[rb];
    total += __popcll(k);
    if (total >= pms) break;   // block-uniform: later rows are cut by post_max_size
    if (tid < m && wave > rb && !sup) {
      const iou3d::Box later = box_at(tid);
      while (k) {
        const int i = base + __ffsll((long long)k) - 1;
        k &= k - 1;
        const iou3d::Box earlier = box_at(i);
        if (iou3d::iou_rotated(earlier, later) > thr) {
          sup = true;
          ssup[tid] = 1;
          break;
        }
      }
    }
  }
  __syncthreads();

  if (tid < m) {
    const unsigned long long w = kept_w[wave];
    if ((w >> lane) & 1ull) {
      int rank = __popcll(w & lanemask_lt());
      for (int q = 0; q < wave; ++q) rank += __popcll(kept_w[q]);
      const int row = sid[tid];
      if (rank < pms && (!post_ok || post_ok[row0 + row])) {   // the range test comes after the cap (centerpoint.py:860-867)
        kflag[row] = 1;
        atomicAdd(&s_count, 1);
      }
    }
  }
  __syncthreads();
  if (tid < R) keep[row0 + tid] = kflag[tid];
  if (tid == 0) counts[s] = s_count;
}

}  // namespace head
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::head;

static int cp_fill_tasks(const char* what, CpTasks& tt, const void* const* heat, const int* classes, int num_tasks, int batch,
                         int height, int width, int max_num) {
  BEVAMD_REQUIRE(classes != nullptr, "%s: the class counts are host arrays and must not be null", what);
  BEVAMD_REQUIRE(num_tasks >= 1 && num_tasks <= CP_MAX_TASKS, "%s: %d tasks (1 .. %d)", what, num_tasks, CP_MAX_TASKS);
  BEVAMD_REQUIRE(batch >= 1 && height >= 1 && width >= 1 && (long long)height * width <= (1 << 24) &&
                     (long long)batch * num_tasks <= 65535,
                 "%s: bad sizes (B %d, T %d, %d x %d)", what, batch, num_tasks, height, width);
  BEVAMD_REQUIRE(max_num >= 1 && max_num <= HE_MAX_K && (long long)max_num <= (long long)height * width,
                 "%s: max_num %d (1 .. %d, at most H*W)", what, max_num, HE_MAX_K);
  tt.T = num_tasks;
  int base = 0;
  for (int t = 0; t < CP_MAX_TASKS; ++t) {
    tt.classes[t] = 0;
    tt.class_base[t] = base;
    tt.heat[t] = nullptr;
    if (t >= num_tasks) continue;
    BEVAMD_REQUIRE(classes[t] >= 1 && classes[t] <= CP_MAX_CLASSES, "%s: task %d has %d classes (1 .. %d)", what, t, classes[t],
                   CP_MAX_CLASSES);
    tt.classes[t] = classes[t];
    if (heat) tt.heat[t] = (const float*)heat[t];
    base += classes[t];
  }
  tt.total_classes = base;
  BEVAMD_REQUIRE((long long)batch * base * height * width <= 0x7fffffffLL, "%s: bad sizes (more than 2^31 cells)", what);
  return BEVAMD_OK;
}

extern "C" {

size_t bevamd_centerpoint_select_workspace_bytes(int batch, int total_classes, int height, int width) {
  if (batch < 1 || total_classes < 1 || height < 1 || width < 1 || (long long)batch * total_classes * height * width > 0x7fffffffLL)
    return 0;
  return align_up((size_t)batch * total_classes * height * width * 8, 256);
}

int bevamd_centerpoint_select(const void* const* heatmaps, const int* task_classes, int num_tasks, int batch, int height, int width,
                              int max_num, int apply_sigmoid, int* top_flat, float* top_score, void* ws, size_t ws_bytes,
                              void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CpTasks tt;
  BEVAMD_REQUIRE(heatmaps != nullptr, "centerpoint_select: the heatmap pointers are a host array and must not be null");
  int rc = cp_fill_tasks("centerpoint_select", tt, heatmaps, task_classes, num_tasks, batch, height, width, max_num);
  if (rc) return rc;
  for (int t = 0; t < num_tasks; ++t) BEVAMD_REQUIRE(tt.heat[t] != nullptr, "centerpoint_select: null heatmap of task %d", t);
  BEVAMD_REQUIRE(top_flat && top_score, "centerpoint_select: null buffer");
  if (!ws || ws_bytes < bevamd_centerpoint_select_workspace_bytes(batch, tt.total_classes, height, width)) {
    set_error("centerpoint_select: workspace too small");
    return BEVAMD_ERR_WORKSPACE;
  }
  const unsigned hw = (unsigned)height * width;
  int cmax = 0;
  for (int t = 0; t < num_tasks; ++t) cmax = tt.classes[t] > cmax ? tt.classes[t] : cmax;
  unsigned long long* cand = (unsigned long long*)ws;
  cp_keys_kernel<<<dim3(cdiv((long long)cmax * hw, 256), batch * num_tasks), dim3(256), 0, stream>>>(tt, hw, apply_sigmoid ? 1 : 0, cand);
  BEVAMD_LAUNCH_CHECK("centerpoint_keys");
  cp_select_kernel<<<dim3(batch * num_tasks), dim3(HE_SEL_THREADS), 0, stream>>>(tt, hw, max_num, cand, top_flat, top_score);
  BEVAMD_LAUNCH_CHECK("centerpoint_select");
  return BEVAMD_OK;
}

int bevamd_centerpoint_decode(const void* const* maps, const int* task_classes, const int* task_rotate, int num_tasks, int batch,
                              int height, int width, int max_num, const int* top_flat, const float* top_score, int norm_bbox, int bottom_centre,
                              const float* coder, const float* post_center_range, float coder_threshold, int use_coder_threshold,
                              float head_threshold, int use_head_threshold, const float* post_center_limit_range, float* boxes,
                              int* labels, unsigned char* live, unsigned char* post_ok, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CpTasks tt;
  int rc = cp_fill_tasks("centerpoint_decode", tt, nullptr, task_classes, num_tasks, batch, height, width, max_num);
  if (rc) return rc;
  BEVAMD_REQUIRE(maps != nullptr, "centerpoint_decode: the map pointers are a host array and must not be null");
  BEVAMD_REQUIRE(coder != nullptr && post_center_range != nullptr,
                 "centerpoint_decode: coder constants and post_center_range are host arrays and must not be null");
  BEVAMD_REQUIRE(top_flat && top_score && boxes && labels && live && post_ok, "centerpoint_decode: null buffer");
  CpMaps mp;
  CpConst cc;
  cc.has_reg = maps[0] != nullptr;
  cc.has_vel = maps[4] != nullptr;
  for (int t = 0; t < CP_MAX_TASKS; ++t) {
    mp.reg[t] = mp.hei[t] = mp.dim[t] = mp.rot[t] = mp.vel[t] = nullptr;
    mp.rotate[t] = 0;
    if (t >= num_tasks) continue;
    const void* const* m = maps + (size_t)t * 5;
    BEVAMD_REQUIRE(m[1] && m[2] && m[3], "centerpoint_decode: null height / dim / rot map of task %d", t);
    BEVAMD_REQUIRE((m[0] != nullptr) == (cc.has_reg != 0) && (m[4] != nullptr) == (cc.has_vel != 0),
                   "centerpoint_decode: reg / vel maps come for every task or for none (task %d)", t);
    mp.reg[t] = (const float*)m[0]; mp.hei[t] = (const float*)m[1]; mp.dim[t] = (const float*)m[2];
    mp.rot[t] = (const float*)m[3]; mp.vel[t] = (const float*)m[4];
    mp.rotate[t] = task_rotate && task_rotate[t] ? 1 : 0;
  }
  cc.osf = coder[0]; cc.vs0 = coder[1]; cc.vs1 = coder[2]; cc.pc0 = coder[3]; cc.pc1 = coder[4];
  cc.has_post = post_center_limit_range ? 1 : 0;
  for (int d = 0; d < 3; ++d) {
    cc.clo[d] = post_center_range[d];
    cc.chi[d] = post_center_range[3 + d];
    cc.plo[d] = post_center_limit_range ? post_center_limit_range[d] : 0.f;
    cc.phi[d] = post_center_limit_range ? post_center_limit_range[3 + d] : 0.f;
  }
  cc.cthr = coder_threshold; cc.use_cthr = use_coder_threshold ? 1 : 0;
  cc.hthr = head_threshold; cc.use_hthr = use_head_threshold ? 1 : 0;
  cc.norm_bbox = norm_bbox ? 1 : 0;
  cc.bottom_centre = bottom_centre ? 1 : 0;
  cp_decode_kernel<<<dim3(cdiv((long long)batch * num_tasks * max_num, 256)), dim3(256), 0, stream>>>(
      tt, mp, cc, batch, height, width, max_num, top_flat, top_score, boxes, labels, live, post_ok);
  BEVAMD_LAUNCH_CHECK("centerpoint_decode");
  return BEVAMD_OK;
}

int bevamd_rotate_nms_segments(const float* boxes, int box_width, const int* labels, const unsigned char* live,
                               const unsigned char* post_ok, int num_segments, int rows_per_segment, int num_tasks,
                               const int* task_enabled, const float* task_thresh, const int* task_label_base, const float* task_scale,
                               int pre_max_size, int post_max_size, unsigned char* keep, int* seg_counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(num_segments >= 0 && rows_per_segment >= 1 && box_width >= 7 && pre_max_size >= 0 && post_max_size >= 0 &&
                     (long long)num_segments * rows_per_segment <= 0x7fffffffLL,
                 "rotate_nms_segments: bad sizes (S %d, rows per segment %d, box width %d, pre_max_size %d, post_max_size %d)",
                 num_segments, rows_per_segment, box_width, pre_max_size, post_max_size);
  BEVAMD_REQUIRE(num_tasks >= 1 && num_tasks <= CP_MAX_TASKS, "rotate_nms_segments: %d tasks (1 .. %d)", num_tasks, CP_MAX_TASKS);
  if (rows_per_segment > HE_MAX_K) {
    set_error("rotate_nms_segments: not supported (segments of %d rows, at most %d)", rows_per_segment, HE_MAX_K);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(task_thresh != nullptr, "rotate_nms_segments: the task tables are host arrays, task_thresh must not be null");
  if (num_segments == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(boxes && keep && seg_counts, "rotate_nms_segments: null buffer");
  BEVAMD_REQUIRE(!task_scale || labels, "rotate_nms_segments: per-class scales need labels");
  CpNms nt;
  nt.T = num_tasks;
  for (int t = 0; t < CP_MAX_TASKS; ++t) {
    const bool in = t < num_tasks;
    nt.enabled[t] = in ? (task_enabled ? (task_enabled[t] ? 1 : 0) : 1) : 0;
    nt.thr[t] = in ? task_thresh[t] : 0.f;
    nt.label_base[t] = in && task_label_base ? task_label_base[t] : 0;
    for (int c = 0; c < CP_MAX_CLASSES; ++c) nt.scale[t][c] = in && task_scale ? task_scale[t * CP_MAX_CLASSES + c] : 1.f;
  }
  rotate_nms_kernel<<<dim3(num_segments), dim3(HE_MAX_K), 0, stream>>>(boxes, box_width, labels, live, post_ok, rows_per_segment,
                                                                      pre_max_size, post_max_size, nt, keep, seg_counts);
  BEVAMD_LAUNCH_CHECK("rotate_nms_segments");
  return BEVAMD_OK;
}

}  // extern "C"
