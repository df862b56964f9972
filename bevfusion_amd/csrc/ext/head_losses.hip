// Losses of the two detection heads, gfx950: forward values and the gradients of every prediction tensor.
//
// Replaces (reference):
//   mmdet3d/models/heads/bbox/transfusion.py:612-711   TransFusionHead.loss: clip_sigmoid + GaussianFocalLoss over the dense map,
//                                                      FocalLoss and L1Loss per decoder layer over permuted / concatenated copies
//   mmdet3d/models/heads/bbox/centerpoint.py:597-633   CenterHead.loss: per task the same dense loss and an L1 over rows gathered
//                                                      from a cat + permute().contiguous() copy of the five regression maps
//   mmdet 2.x gaussian_focal_loss, py_sigmoid_focal_loss, l1_loss with weight_reduce_loss(reduction="mean", avg_factor)
//
// Native formulation:
//   * gf_kernel<false>   dense Gaussian focal loss of up to 16 maps in one launch: a workgroup owns passes of HL_SHARE cells of one
//                        map (16-byte loads of the prediction between a scalar head and tail), sums the cell losses and the
//                        count of target == 1 in fp64 and writes one (sum, count) partial;
//   * gf_finish_kernel   one workgroup per map adds the map's partials in a fixed order: num_pos, avg and the loss;
//   * gf_kernel<true>    the gradient of every cell recomputed from logit and target (the forward saves nothing dense);
//   * layer_kernel       one workgroup per (decoder layer, loss): sigmoid focal loss of the class scores read in place from
//                        [B, C, L * K], and the L1 of the five box pieces read in place from [B, c, L * K];
//   * layer_grad_kernel  their gradients, element-wise, every element written;
//   * chbox_kernel       CenterHead box L1: one workgroup per task reads the five maps only at ind[b, m];
//   * zero_maps_kernel, chbox_scatter_kernel   its gradient: the maps are zeroed inside the call, then one workgroup per (sample,
//                        task) stages the slot terms in LDS and the FIRST slot of every group of slots sharing a cell writes the
//                        group's fp32 sum, taken in slot order (an O(M^2) scan as slots_kernel of head_targets.hip).
// Launches: gaussian focal forward 2, backward 1; layer losses forward 1, backward 1; CenterHead box forward 1, backward 2.
// Every cell term is evaluated in double from the fp32 inputs (sigmoid, log, pow: no intermediate fp32 rounding), accumulated in
// fp64 and combined in a fixed order; the mean and the loss weight are the reference's fp32 operations: loss_weight * (sum / avg).
// The products the reference rounds to fp32 before they meet the data (bbox_weights * code_weights) are rounded here too.  No
// floating-point atomics, no workspace besides the typed partial buffer, nothing read back.  fp contract(off).
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace bevamd {
namespace head_losses {

constexpr int HL_THREADS = 256;
constexpr int HL_SHARE = 2048;       // cells of one workgroup pass
constexpr int HL_GRID_CAP = 1024;    // workgroups per map: a larger map is walked in several passes
constexpr int HL_MAX_MAPS = 16;
constexpr int HL_MAX_SLOTS = 1024;   // max_objs of the CenterHead box loss
constexpr int HL_MAX_CODE = 16;      // columns of a packed L1 problem

static int plan_workgroups(long long cells) {
  const long long w = (cells + HL_SHARE - 1) / HL_SHARE;
  return (int)(w < HL_GRID_CAP ? w : HL_GRID_CAP);
}

// ---- helpers ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double hl_pow(double v, double e) {
  if (e == 2.0) return v * v;
  if (e == 4.0) return (v * v) * (v * v);
  if (e == 1.0) return v;
  return pow(v, e);
}

// the sum of v over the workgroup, in a fixed order; s: HL_THREADS doubles
__device__ __forceinline__ double block_sum(double v, double* s) {
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int o = HL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  return s[0];
}

// ---- Gaussian focal loss ------------------------------------------------------------------------------------------------------
struct GfArgs {
  int num_maps, pred_is_logit, partial_stride;
  float loss_weight;
  double alpha, gamma;
  const float* pred[HL_MAX_MAPS];
  const float* target[HL_MAX_MAPS];
  const float* avg[HL_MAX_MAPS];     // optional device scalar per map
  float* grad[HL_MAX_MAPS];
  long long cells[HL_MAX_MAPS];
  int wg_first[HL_MAX_MAPS + 1];     // map t owns the workgroups [wg_first[t], wg_first[t + 1])
};

// p of one cell and whether the clamp of clip_sigmoid is active (torch passes the gradient on the closed interval)
__device__ __forceinline__ double gf_prob(float x, int is_logit, bool& clamped) {
  clamped = false;
  if (!is_logit) return (double)x;
  double p = 1.0 / (1.0 + exp(-(double)x));
  const double lo = 1e-4, hi = 1.0 - 1e-4;
  if (p < lo) {
    p = lo;
    clamped = true;
  } else if (p > hi) {
    p = hi;
    clamped = true;
  }
  return p;                           // a NaN stays a NaN
}

__device__ __forceinline__ double gf_loss(float x, float t, const GfArgs& a) {
  bool clamped;
  const double p = gf_prob(x, a.pred_is_logit, clamped);
  const double eps = 1e-12;
  const double pos = t == 1.f ? 1.0 : 0.0;
  const double neg = hl_pow(1.0 - (double)t, a.gamma);
  return -log(p + eps) * hl_pow(1.0 - p, a.alpha) * pos + -log(1.0 - p + eps) * hl_pow(p, a.alpha) * neg;
}

// d loss / d x (d p with pred_is_logit 0)
__device__ __forceinline__ double gf_dloss(float x, float t, const GfArgs& a) {
  bool clamped;
  const double p = gf_prob(x, a.pred_is_logit, clamped);
  if (clamped) return 0.0;
  const double eps = 1e-12;
  const double pos = t == 1.f ? 1.0 : 0.0;
  const double neg = hl_pow(1.0 - (double)t, a.gamma);
  const double q = 1.0 - p;
  const double dpos = -hl_pow(q, a.alpha) / (p + eps) + a.alpha * hl_pow(q, a.alpha - 1.0) * log(p + eps);
  const double dneg = hl_pow(p, a.alpha) / (q + eps) - a.alpha * hl_pow(p, a.alpha - 1.0) * log(q + eps);
  const double d = dpos * pos + dneg * neg;
  return a.pred_is_logit ? d * (p * q) : d;
}

template <bool BWD>
__global__ __launch_bounds__(HL_THREADS) void gf_kernel(GfArgs a, double* __restrict__ partials, const float* __restrict__ num_pos,
                                                        const float* __restrict__ grad_out) {
  __shared__ double s_red[HL_THREADS];
  const int tid = threadIdx.x;
  int t = 0;
  while (t + 1 < a.num_maps && (int)blockIdx.x >= a.wg_first[t + 1]) ++t;
  const int w = blockIdx.x - a.wg_first[t], nwg = a.wg_first[t + 1] - a.wg_first[t];
  const float* __restrict__ x = a.pred[t];
  const float* __restrict__ tg = a.target[t];
  float* __restrict__ g = a.grad[t];
  const long long n = a.cells[t];
  float scale = 0.f;
  if (BWD) {
    const float avg = a.avg[t] != nullptr ? *a.avg[t] : fmaxf(num_pos[t], 1.f);
    scale = grad_out[t] * a.loss_weight / avg;
  }
  double sum = 0.0, cnt = 0.0;
  for (long long start = (long long)w * HL_SHARE; start < n; start += (long long)nwg * HL_SHARE) {
    const int len = (int)(n - start < HL_SHARE ? n - start : HL_SHARE);
    const float* xs = x + start;
    const float* ts = tg + start;
    float* gs = BWD ? g + start : nullptr;
    // 16-byte accesses on the prediction (and the gradient, which must share its alignment) between a scalar head up to the
    // boundary and a scalar tail; the target, a view into the heads' one heatmap buffer, is read wide where it is aligned there too
    const unsigned mis = (unsigned)((uintptr_t)xs & 15u);
    const bool wide = !BWD || ((uintptr_t)gs & 15u) == mis;
    int head = wide ? (int)(((16u - mis) & 15u) >> 2) : len;
    if (head > len) head = len;
    const int quads = (len - head) >> 2;
    const int tail = head + (quads << 2);
    const bool target_wide = ((uintptr_t)(ts + head) & 15u) == 0;
    for (int i = tid; i < head; i += HL_THREADS) {
      if (BWD) {
        gs[i] = (float)gf_dloss(xs[i], ts[i], a) * scale;
      } else {
        sum += gf_loss(xs[i], ts[i], a);
        cnt += ts[i] == 1.f ? 1.0 : 0.0;
      }
    }
    for (int q = tid; q < quads; q += HL_THREADS) {
      const float4 xv = *reinterpret_cast<const float4*>(xs + head + 4 * q);
      float4 tv;
      if (target_wide) {
        tv = *reinterpret_cast<const float4*>(ts + head + 4 * q);
      } else {
        const float* tp = ts + head + 4 * q;
        tv.x = tp[0], tv.y = tp[1], tv.z = tp[2], tv.w = tp[3];
      }
      if (BWD) {
        float4 o;
        o.x = (float)gf_dloss(xv.x, tv.x, a) * scale;
        o.y = (float)gf_dloss(xv.y, tv.y, a) * scale;
        o.z = (float)gf_dloss(xv.z, tv.z, a) * scale;
        o.w = (float)gf_dloss(xv.w, tv.w, a) * scale;
        *reinterpret_cast<float4*>(gs + head + 4 * q) = o;
      } else {
        sum += gf_loss(xv.x, tv.x, a);
        sum += gf_loss(xv.y, tv.y, a);
        sum += gf_loss(xv.z, tv.z, a);
        sum += gf_loss(xv.w, tv.w, a);
        cnt += (tv.x == 1.f ? 1.0 : 0.0) + (tv.y == 1.f ? 1.0 : 0.0) + (tv.z == 1.f ? 1.0 : 0.0) + (tv.w == 1.f ? 1.0 : 0.0);
      }
    }
    for (int i = tail + tid; i < len; i += HL_THREADS) {
      if (BWD) {
        gs[i] = (float)gf_dloss(xs[i], ts[i], a) * scale;
      } else {
        sum += gf_loss(xs[i], ts[i], a);
        cnt += ts[i] == 1.f ? 1.0 : 0.0;
      }
    }
  }
  if (!BWD) {
    const double s = block_sum(sum, s_red);
    const double c = block_sum(cnt, s_red);
    if (tid == 0) {
      double* out = partials + ((size_t)t * a.partial_stride + w) * 2;
      out[0] = s;
      out[1] = c;
    }
  }
}

__global__ __launch_bounds__(HL_THREADS) void gf_finish_kernel(GfArgs a, const double* __restrict__ partials, float* __restrict__ loss,
                                                               float* __restrict__ num_pos) {
  __shared__ double s_red[HL_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int nwg = a.wg_first[t + 1] - a.wg_first[t];
  const double* in = partials + (size_t)t * a.partial_stride * 2;
  double sum = 0.0, cnt = 0.0;
  for (int w = tid; w < nwg; w += HL_THREADS) {
    sum += in[2 * w];
    cnt += in[2 * w + 1];
  }
  const double s = block_sum(sum, s_red);
  const double c = block_sum(cnt, s_red);
  if (tid == 0) {
    const float np = (float)c;
    const float avg = a.avg[t] != nullptr ? *a.avg[t] : fmaxf(np, 1.f);
    num_pos[t] = np;
    loss[t] = a.loss_weight * ((float)s / avg);
  }
}

static int gf_fill(GfArgs& a, const char* what, const float* const* pred, const float* const* target, const long long* cells,
                   int num_maps, int pred_is_logit, double alpha, double gamma, float loss_weight, const float* const* avg,
                   float* const* grad) {
  BEVAMD_REQUIRE(num_maps >= 1 && num_maps <= HL_MAX_MAPS, "%s: %d maps (1 .. %d)", what, num_maps, HL_MAX_MAPS);
  BEVAMD_REQUIRE(pred != nullptr && target != nullptr && cells != nullptr, "%s: pred, target and cells are host arrays of %d entries",
                 what, num_maps);
  a = GfArgs{};
  a.num_maps = num_maps;
  a.pred_is_logit = pred_is_logit ? 1 : 0;
  a.loss_weight = loss_weight;
  a.alpha = alpha;
  a.gamma = gamma;
  long long largest = 0;
  int total = 0;
  for (int t = 0; t < num_maps; ++t) {
    BEVAMD_REQUIRE(cells[t] >= 1 && cells[t] <= (1LL << 40), "%s: map %d has %lld cells", what, t, cells[t]);
    BEVAMD_REQUIRE(pred[t] != nullptr && target[t] != nullptr && (grad == nullptr || grad[t] != nullptr), "%s: null pointer (map %d)",
                   what, t);
    BEVAMD_REQUIRE((((uintptr_t)pred[t] | (uintptr_t)target[t] | (uintptr_t)(grad ? grad[t] : nullptr)) & 3u) == 0,
                   "%s: map %d is not 4-byte aligned", what, t);
    a.pred[t] = pred[t];
    a.target[t] = target[t];
    a.avg[t] = avg != nullptr ? avg[t] : nullptr;
    a.grad[t] = grad != nullptr ? grad[t] : nullptr;
    a.cells[t] = cells[t];
    a.wg_first[t] = total;
    total += plan_workgroups(cells[t]);
    if (cells[t] > largest) largest = cells[t];
  }
  a.wg_first[num_maps] = total;
  a.partial_stride = plan_workgroups(largest);
  return BEVAMD_OK;
}

// ---- per-layer losses of the TransFusion head -----------------------------------------------------------------------------------
struct LayerArgs {
  const float* scores;               // [B, C, L * K], or null: no class loss
  const long long* labels;           // [B, L * K]
  const void* label_weights;         // [B, L * K] fp32 (dtype 0) or int64 (dtype 2)
  int weight_dtype;
  const float* piece[5];             // center [B, 2, P], height [B, 1, P], dim [B, 3, P], rot [B, 2, P], vel [B, 2, P] or null; packed: piece[0] is [B, P, D]
  int packed;
  const float* bbox_targets;         // [B, P, D]
  const float* bbox_weights;
  float code_weights[HL_MAX_CODE];
  const int* num_pos;                // avg = max(num_pos, 1) ...
  const float* avg_cls;              // ... unless a device scalar is given
  const float* avg_box;
  int B, C, L, K, D;
  double alpha, gamma;
  float cls_weight, box_weight;
};

__device__ __forceinline__ float layer_avg(const int* num_pos, const float* avg) {
  if (avg != nullptr) return *avg;
  const int n = *num_pos;
  return (float)(n > 1 ? n : 1);
}

__device__ __forceinline__ double layer_weight(const LayerArgs& a, size_t i) {
  return a.weight_dtype == 0 ? (double)((const float*)a.label_weights)[i] : (double)((const long long*)a.label_weights)[i];
}

// py_sigmoid_focal_loss of one element: the value, or its derivative in x.  y outside {0, 1} is never passed.
__device__ __forceinline__ double focal_term(float xf, double y, double alpha, double gamma, bool derivative) {
  const double x = (double)xf;
  const double s = 1.0 / (1.0 + exp(-x));
  const double pt = (1.0 - s) * y + s * (1.0 - y);
  const double at = alpha * y + (1.0 - alpha) * (1.0 - y);
  const double bce = (1.0 - y) * x + (fmax(-x, 0.0) + log1p(exp(-fabs(x))));   // binary_cross_entropy_with_logits
  if (!derivative) return bce * (at * hl_pow(pt, gamma));
  const double dpt = s * (1.0 - s) * (1.0 - 2.0 * y);
  return (s - y) * (at * hl_pow(pt, gamma)) + bce * (at * gamma * hl_pow(pt, gamma - 1.0) * dpt);
}

// the column of code d in the pieces: piece index and the channel inside it
__device__ __forceinline__ void code_piece(int d, int& piece, int& ch, int& width) {
  if (d < 2) {
    piece = 0, ch = d, width = 2;
  } else if (d < 3) {
    piece = 1, ch = 0, width = 1;
  } else if (d < 6) {
    piece = 2, ch = d - 3, width = 3;
  } else if (d < 8) {
    piece = 3, ch = d - 6, width = 2;
  } else {
    piece = 4, ch = d - 8, width = 2;
  }
}

__device__ __forceinline__ size_t box_pred_index(const LayerArgs& a, int b, int p, int d, int& piece) {
  const int P = a.L * a.K;
  if (a.packed) {
    piece = 0;
    return ((size_t)b * P + p) * a.D + d;
  }
  int ch, width;
  code_piece(d, piece, ch, width);
  return ((size_t)b * width + ch) * P + p;
}

// grid 2 L: workgroup l < L the class loss of layer l, workgroup L + l its box loss
__global__ __launch_bounds__(HL_THREADS) void layer_kernel(LayerArgs a, float* __restrict__ loss_cls, float* __restrict__ loss_box) {
  __shared__ double s_red[HL_THREADS];
  const int tid = threadIdx.x;
  const int P = a.L * a.K;
  const bool cls = (int)blockIdx.x < a.L;
  const int l = cls ? blockIdx.x : blockIdx.x - a.L;
  double sum = 0.0;
  if (cls) {
    if (a.scores == nullptr) return;
    const long long n = (long long)a.B * a.C * a.K;
    for (long long e = tid; e < n; e += HL_THREADS) {
      const int k = (int)(e % a.K);
      const int c = (int)((e / a.K) % a.C);
      const int b = (int)(e / ((long long)a.K * a.C));
      const size_t row = (size_t)b * P + (size_t)l * a.K + k;
      const long long label = a.labels[row];
      if (label < 0 || label > a.C) {
        sum += (double)NAN;           // no row of the one-hot matrix
        continue;
      }
      const float x = a.scores[((size_t)b * a.C + c) * P + (size_t)l * a.K + k];
      sum += focal_term(x, label == c ? 1.0 : 0.0, a.alpha, a.gamma, false) * layer_weight(a, row);
    }
    const double s = block_sum(sum, s_red);
    if (tid == 0) loss_cls[l] = a.cls_weight * ((float)s / layer_avg(a.num_pos, a.avg_cls));
  } else {
    if (a.piece[0] == nullptr) return;
    const long long n = (long long)a.B * a.D * a.K;
    for (long long e = tid; e < n; e += HL_THREADS) {
      const int k = (int)(e % a.K);
      const int d = (int)((e / a.K) % a.D);
      const int b = (int)(e / ((long long)a.K * a.D));
      const int p = l * a.K + k;
      int piece;
      const size_t at = box_pred_index(a, b, p, d, piece);
      const size_t tt = ((size_t)b * P + p) * a.D + d;
      const float w = a.bbox_weights[tt] * a.code_weights[d];          // layer_reg_weights, an fp32 tensor
      sum += fabs((double)a.piece[piece][at] - (double)a.bbox_targets[tt]) * (double)w;
    }
    const double s = block_sum(sum, s_red);
    if (tid == 0) loss_box[l] = a.box_weight * ((float)s / layer_avg(a.num_pos, a.avg_box));
  }
}

// one thread per element of grad_scores [B, C, P], then per element of the box gradients (b, d, p)
__global__ __launch_bounds__(HL_THREADS) void layer_grad_kernel(LayerArgs a, const float* __restrict__ grad_cls,
                                                                const float* __restrict__ grad_box, float* __restrict__ grad_scores,
                                                                float* g0, float* g1, float* g2, float* g3, float* g4) {
  const int P = a.L * a.K;
  const long long n_cls = a.scores != nullptr ? (long long)a.B * a.C * P : 0;
  const long long n_box = a.piece[0] != nullptr ? (long long)a.B * a.D * P : 0;
  const long long stride = (long long)gridDim.x * HL_THREADS;
  for (long long e = (long long)blockIdx.x * HL_THREADS + threadIdx.x; e < n_cls + n_box; e += stride) {
    if (e < n_cls) {
      const int p = (int)(e % P);
      const int c = (int)((e / P) % a.C);
      const int b = (int)(e / ((long long)P * a.C));
      const size_t row = (size_t)b * P + p;
      const long long label = a.labels[row];
      const float scale = grad_cls[p / a.K] * a.cls_weight / layer_avg(a.num_pos, a.avg_cls);
      float g;
      if (label < 0 || label > a.C) {
        g = NAN;
      } else {
        const double d = focal_term(a.scores[e], label == c ? 1.0 : 0.0, a.alpha, a.gamma, true);
        g = (float)(d * layer_weight(a, row)) * scale;
      }
      grad_scores[e] = g;
    } else {
      const long long r = e - n_cls;
      const int p = (int)(r % P);
      const int d = (int)((r / P) % a.D);
      const int b = (int)(r / ((long long)P * a.D));
      int piece;
      const size_t at = box_pred_index(a, b, p, d, piece);
      const size_t tt = ((size_t)b * P + p) * a.D + d;
      const float w = a.bbox_weights[tt] * a.code_weights[d];
      const float diff = a.piece[piece][at] - a.bbox_targets[tt];
      const float sign = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : diff);   // sign(0) = 0, sign(NaN) = NaN
      const float scale = grad_box[p / a.K] * a.box_weight / layer_avg(a.num_pos, a.avg_box);
      float* out = piece == 0 ? g0 : piece == 1 ? g1 : piece == 2 ? g2 : piece == 3 ? g3 : g4;
      out[at] = (scale * w) * sign;
    }
  }
}

// ---- CenterHead box loss ------------------------------------------------------------------------------------------------------
struct ChArgs {
  const float* maps[HL_MAX_MAPS][5];   // reg [B, 2, HW], height [B, 1, HW], dim [B, 3, HW], rot [B, 2, HW], vel [B, 2, HW]
  float* grads[HL_MAX_MAPS][5];
  const long long* ind[HL_MAX_MAPS];   // [B, M]
  const float* target[HL_MAX_MAPS];    // [B, M, 10]
  const unsigned char* mask[HL_MAX_MAPS];
  int T, B, M;
  long long hw;
  float code_weights[10];
  float loss_weight;
};

__device__ __forceinline__ float ch_pred(const float* const* maps, int b, long long cell, long long hw, int d) {
  int piece, ch, width;
  code_piece(d, piece, ch, width);
  return maps[piece][((size_t)b * width + ch) * hw + cell];
}

// grid T: the loss and avg = mask.sum() + 1e-4 of one task
__global__ __launch_bounds__(HL_THREADS) void chbox_kernel(ChArgs a, float* __restrict__ loss, float* __restrict__ avg_out) {
  __shared__ double s_red[HL_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int slots = a.B * a.M;
  double sum = 0.0, live = 0.0;
  for (int s = tid; s < slots; s += HL_THREADS) {
    const int b = s / a.M;
    const long long cell = a.ind[t][s];
    const float m = a.mask[t][s] ? 1.f : 0.f;
    live += (double)m;
    if (cell < 0 || cell >= a.hw) {
      sum += (double)NAN;              // an index outside the map: nothing is read
      continue;
    }
    const float* tg = a.target[t] + (size_t)s * 10;
    for (int d = 0; d < 10; ++d) {
      const float tv = tg[d];
      const float w = (m * (tv != tv ? 0.f : 1.f)) * a.code_weights[d];
      sum += fabs((double)ch_pred(a.maps[t], b, cell, a.hw, d) - (double)tv) * (double)w;
    }
  }
  const double s = block_sum(sum, s_red);
  const double c = block_sum(live, s_red);
  if (tid == 0) {
    const float avg = (float)c + 1e-4f;
    avg_out[t] = avg;
    loss[t] = a.loss_weight * ((float)s / avg);
  }
}

// grid (chunks, 5 T): zero every gradient map
__global__ __launch_bounds__(HL_THREADS) void zero_maps_kernel(ChArgs a) {
  const int t = blockIdx.y / 5, piece = blockIdx.y % 5;
  const int width = piece == 1 ? 1 : (piece == 2 ? 3 : 2);
  float* g = a.grads[t][piece];
  const long long n = (long long)a.B * width * a.hw;
  const long long stride = (long long)gridDim.x * HL_THREADS;
  for (long long i = (long long)blockIdx.x * HL_THREADS + threadIdx.x; i < n; i += stride) g[i] = 0.f;
}

// grid (B, T): slots sharing a cell are summed in slot order by the first of them
__global__ __launch_bounds__(HL_THREADS) void chbox_scatter_kernel(ChArgs a, const float* __restrict__ avg, const float* __restrict__ grad_out) {
  __shared__ int s_cell[HL_MAX_SLOTS];
  __shared__ float s_term[HL_MAX_SLOTS * 10];
  const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const float scale = grad_out[t] * a.loss_weight / avg[t];
  for (int m = tid; m < a.M; m += HL_THREADS) {
    const size_t s = (size_t)b * a.M + m;
    const long long cell = a.ind[t][s];
    const bool inside = cell >= 0 && cell < a.hw;
    s_cell[m] = inside ? (int)cell : -1;
    const float mk = a.mask[t][s] ? 1.f : 0.f;
    const float* tg = a.target[t] + s * 10;
    for (int d = 0; d < 10; ++d) {
      float term = 0.f;
      if (inside) {
        const float tv = tg[d];
        const float w = (mk * (tv != tv ? 0.f : 1.f)) * a.code_weights[d];
        const float diff = ch_pred(a.maps[t], b, cell, a.hw, d) - tv;
        const float sign = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : diff);
        term = (scale * w) * sign;
      }
      s_term[m * 10 + d] = term;
    }
  }
  __syncthreads();
  for (int m = tid; m < a.M; m += HL_THREADS) {
    const int cell = s_cell[m];
    if (cell < 0) continue;
    bool first = true;
    for (int j = 0; j < m; ++j)
      if (s_cell[j] == cell) {
        first = false;
        break;
      }
    if (!first) continue;
    float acc[10];
    for (int d = 0; d < 10; ++d) acc[d] = s_term[m * 10 + d];
    for (int j = m + 1; j < a.M; ++j) {
      if (s_cell[j] != cell) continue;
      for (int d = 0; d < 10; ++d) acc[d] += s_term[j * 10 + d];
    }
    for (int d = 0; d < 10; ++d) {
      int piece, ch, width;
      code_piece(d, piece, ch, width);
      a.grads[t][piece][((size_t)b * width + ch) * a.hw + cell] = acc[d];
    }
  }
}

static int ch_fill(ChArgs& a, const char* what, const float* const* maps, const long long* const* ind, const float* const* target,
                   const unsigned char* const* mask, int T, int B, int M, long long hw, const float* code_weights, float loss_weight,
                   float* const* grads) {
  BEVAMD_REQUIRE(T >= 1 && T <= HL_MAX_MAPS, "%s: %d tasks (1 .. %d)", what, T, HL_MAX_MAPS);
  BEVAMD_REQUIRE(B >= 1 && B <= 65535 && M >= 1 && hw >= 1 && hw <= 0x7fffffffLL, "%s: bad sizes (batch %d, max_objs %d, cells %lld)",
                 what, B, M, hw);
  if (M > HL_MAX_SLOTS) {
    set_error("%s: max_objs %d (1 .. %d)", what, M, HL_MAX_SLOTS);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  BEVAMD_REQUIRE(maps != nullptr && ind != nullptr && target != nullptr && mask != nullptr && code_weights != nullptr,
                 "%s: maps [5 * tasks], ind, target, mask [tasks] and code_weights [10] are host arrays", what);
  a = ChArgs{};
  for (int t = 0; t < T; ++t) {
    BEVAMD_REQUIRE(ind[t] != nullptr && target[t] != nullptr && mask[t] != nullptr, "%s: null pointer (task %d)", what, t);
    for (int p = 0; p < 5; ++p) {
      BEVAMD_REQUIRE(maps[5 * t + p] != nullptr && (grads == nullptr || grads[5 * t + p] != nullptr), "%s: null map (task %d, piece %d)",
                     what, t, p);
      a.maps[t][p] = maps[5 * t + p];
      a.grads[t][p] = grads != nullptr ? grads[5 * t + p] : nullptr;
    }
    a.ind[t] = ind[t];
    a.target[t] = target[t];
    a.mask[t] = mask[t];
  }
  a.T = T;
  a.B = B;
  a.M = M;
  a.hw = hw;
  for (int d = 0; d < 10; ++d) a.code_weights[d] = code_weights[d];
  a.loss_weight = loss_weight;
  return BEVAMD_OK;
}

static int layer_fill(LayerArgs& a, const char* what, const float* scores, const long long* labels, const void* label_weights,
                      int weight_dtype, const float* center, const float* height, const float* dim, const float* rot, const float* vel,
                      const float* bbox_targets, const float* bbox_weights, const float* code_weights, const int* num_pos,
                      const float* avg_cls, const float* avg_box, int B, int C, int L, int K, int D, double alpha, double gamma,
                      float cls_weight, float box_weight) {
  BEVAMD_REQUIRE(B >= 1 && L >= 1 && K >= 1 && (long long)B * L * K <= 0x7fffffffLL / 64, "%s: bad sizes (batch %d, layers %d, proposals %d)",
                 what, B, L, K);
  BEVAMD_REQUIRE(scores != nullptr || center != nullptr, "%s: neither class scores nor boxes", what);
  a = LayerArgs{};
  if (scores != nullptr) {
    BEVAMD_REQUIRE(C >= 1 && C <= 64, "%s: %d classes (1 .. 64)", what, C);
    BEVAMD_REQUIRE(labels != nullptr && label_weights != nullptr, "%s: null pointer (labels, label_weights)", what);
    if (weight_dtype != 0 && weight_dtype != 2) {
      set_error("%s: label_weights dtype code %d (0 fp32, 2 int64)", what, weight_dtype);
      return BEVAMD_ERR_UNSUPPORTED;
    }
    BEVAMD_REQUIRE(num_pos != nullptr || avg_cls != nullptr, "%s: num_pos or avg_cls", what);
  }
  if (center != nullptr) {
    const bool packed = height == nullptr && dim == nullptr && rot == nullptr && vel == nullptr;
    if (packed) {
      BEVAMD_REQUIRE(D >= 1 && D <= HL_MAX_CODE, "%s: a packed box tensor has 1 .. %d columns, got %d", what, HL_MAX_CODE, D);
    } else {
      BEVAMD_REQUIRE(D == 8 || D == 10, "%s: the code has 8 or 10 columns, got %d", what, D);
      BEVAMD_REQUIRE(height != nullptr && dim != nullptr && rot != nullptr && (vel != nullptr) == (D == 10),
                     "%s: center, height, dim, rot and (with 10 columns only) vel", what);
    }
    BEVAMD_REQUIRE(bbox_targets != nullptr && bbox_weights != nullptr, "%s: null pointer (bbox_targets, bbox_weights)", what);
    BEVAMD_REQUIRE(num_pos != nullptr || avg_box != nullptr, "%s: num_pos or avg_box", what);
    a.packed = packed ? 1 : 0;
    for (int d = 0; d < HL_MAX_CODE; ++d) a.code_weights[d] = (code_weights != nullptr && d < D) ? code_weights[d] : 1.f;
  }
  a.scores = scores;
  a.labels = labels;
  a.label_weights = label_weights;
  a.weight_dtype = weight_dtype;
  a.piece[0] = center;
  a.piece[1] = height;
  a.piece[2] = dim;
  a.piece[3] = rot;
  a.piece[4] = vel;
  a.bbox_targets = bbox_targets;
  a.bbox_weights = bbox_weights;
  a.num_pos = num_pos;
  a.avg_cls = avg_cls;
  a.avg_box = avg_box;
  a.B = B, a.C = scores != nullptr ? C : 1, a.L = L, a.K = K, a.D = center != nullptr ? D : 1;
  a.alpha = alpha, a.gamma = gamma;
  a.cls_weight = cls_weight, a.box_weight = box_weight;
  return BEVAMD_OK;
}

}  // namespace head_losses
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::head_losses;

extern "C" {

int bevamd_head_loss_plan(long long cells, int* plan2) {
  BEVAMD_REQUIRE(plan2 != nullptr && cells >= 1 && cells <= (1LL << 40), "head_loss_plan: %lld cells (1 .. 2^40), plan2 a host array",
                 cells);
  plan2[0] = plan_workgroups(cells);
  plan2[1] = HL_SHARE;
  return BEVAMD_OK;
}

int bevamd_gaussian_focal_forward(const float* const* pred, const float* const* target, const long long* cells, int num_maps,
                                  int pred_is_logit, double alpha, double gamma, float loss_weight, const float* const* avg,
                                  double* partials, float* loss, float* num_pos, void* stream) {
  GfArgs a;
  const int rc = gf_fill(a, "gaussian_focal_forward", pred, target, cells, num_maps, pred_is_logit, alpha, gamma, loss_weight, avg, nullptr);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(partials != nullptr && loss != nullptr && num_pos != nullptr, "gaussian_focal_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gf_kernel<false>, dim3(a.wg_first[num_maps]), dim3(HL_THREADS), 0, s, a, partials, (const float*)nullptr,
                     (const float*)nullptr);
  BEVAMD_LAUNCH_CHECK("gaussian_focal partials");
  hipLaunchKernelGGL(gf_finish_kernel, dim3(num_maps), dim3(HL_THREADS), 0, s, a, (const double*)partials, loss, num_pos);
  BEVAMD_LAUNCH_CHECK("gaussian_focal finish");
  return BEVAMD_OK;
}

int bevamd_gaussian_focal_backward(const float* const* pred, const float* const* target, const long long* cells, int num_maps,
                                   int pred_is_logit, double alpha, double gamma, float loss_weight, const float* const* avg,
                                   const float* num_pos, const float* grad_out, float* const* grad, void* stream) {
  GfArgs a;
  BEVAMD_REQUIRE(grad != nullptr, "gaussian_focal_backward: grad is a host array of device pointers");
  const int rc = gf_fill(a, "gaussian_focal_backward", pred, target, cells, num_maps, pred_is_logit, alpha, gamma, loss_weight, avg, grad);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(num_pos != nullptr && grad_out != nullptr, "gaussian_focal_backward: null pointer");
  hipLaunchKernelGGL(gf_kernel<true>, dim3(a.wg_first[num_maps]), dim3(HL_THREADS), 0, (hipStream_t)stream, a, (double*)nullptr, num_pos,
                     grad_out);
  BEVAMD_LAUNCH_CHECK("gaussian_focal backward");
  return BEVAMD_OK;
}

int bevamd_transfusion_layer_losses_forward(const float* scores, const long long* labels, const void* label_weights, int weight_dtype,
                                            const float* center, const float* height, const float* dim, const float* rot,
                                            const float* vel, const float* bbox_targets, const float* bbox_weights,
                                            const float* code_weights, const int* num_pos, const float* avg_cls, const float* avg_box,
                                            int B, int C, int L, int K, int D, double alpha, double gamma, float cls_weight,
                                            float box_weight, float* loss_cls, float* loss_box, void* stream) {
  LayerArgs a;
  const int rc = layer_fill(a, "transfusion_layer_losses_forward", scores, labels, label_weights, weight_dtype, center, height, dim, rot,
                            vel, bbox_targets, bbox_weights, code_weights, num_pos, avg_cls, avg_box, B, C, L, K, D, alpha, gamma,
                            cls_weight, box_weight);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE((scores == nullptr || loss_cls != nullptr) && (center == nullptr || loss_box != nullptr),
                 "transfusion_layer_losses_forward: null output");
  hipLaunchKernelGGL(layer_kernel, dim3(2 * L), dim3(HL_THREADS), 0, (hipStream_t)stream, a, loss_cls, loss_box);
  BEVAMD_LAUNCH_CHECK("transfusion_layer_losses forward");
  return BEVAMD_OK;
}

int bevamd_transfusion_layer_losses_backward(const float* scores, const long long* labels, const void* label_weights, int weight_dtype,
                                             const float* center, const float* height, const float* dim, const float* rot,
                                             const float* vel, const float* bbox_targets, const float* bbox_weights,
                                             const float* code_weights, const int* num_pos, const float* avg_cls, const float* avg_box,
                                             int B, int C, int L, int K, int D, double alpha, double gamma, float cls_weight,
                                             float box_weight, const float* grad_cls, const float* grad_box, float* grad_scores,
                                             float* grad_center, float* grad_height, float* grad_dim, float* grad_rot, float* grad_vel,
                                             void* stream) {
  LayerArgs a;
  const int rc = layer_fill(a, "transfusion_layer_losses_backward", scores, labels, label_weights, weight_dtype, center, height, dim, rot,
                            vel, bbox_targets, bbox_weights, code_weights, num_pos, avg_cls, avg_box, B, C, L, K, D, alpha, gamma,
                            cls_weight, box_weight);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(scores == nullptr || (grad_cls != nullptr && grad_scores != nullptr), "transfusion_layer_losses_backward: null pointer (class)");
  if (center != nullptr) {
    BEVAMD_REQUIRE(grad_box != nullptr && grad_center != nullptr, "transfusion_layer_losses_backward: null pointer (boxes)");
    BEVAMD_REQUIRE(a.packed || (grad_height != nullptr && grad_dim != nullptr && grad_rot != nullptr && (grad_vel != nullptr) == (D == 10)),
                   "transfusion_layer_losses_backward: one gradient per piece");
  }
  const long long n = (long long)B * L * K * ((scores != nullptr ? a.C : 0) + (center != nullptr ? a.D : 0));
  const int grid = (int)((n + HL_THREADS - 1) / HL_THREADS < 4096 ? (n + HL_THREADS - 1) / HL_THREADS : 4096);
  hipLaunchKernelGGL(layer_grad_kernel, dim3(grid), dim3(HL_THREADS), 0, (hipStream_t)stream, a, grad_cls, grad_box, grad_scores,
                     grad_center, grad_height, grad_dim, grad_rot, grad_vel);
  BEVAMD_LAUNCH_CHECK("transfusion_layer_losses backward");
  return BEVAMD_OK;
}

int bevamd_centerhead_box_loss_forward(const float* const* maps, const long long* const* ind, const float* const* target,
                                       const unsigned char* const* mask, int num_tasks, int batch, int max_objs, long long hw,
                                       const float* code_weights, float loss_weight, float* loss, float* avg, void* stream) {
  ChArgs a;
  const int rc = ch_fill(a, "centerhead_box_loss_forward", maps, ind, target, mask, num_tasks, batch, max_objs, hw, code_weights, loss_weight,
                         nullptr);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(loss != nullptr && avg != nullptr, "centerhead_box_loss_forward: null pointer");
  hipLaunchKernelGGL(chbox_kernel, dim3(num_tasks), dim3(HL_THREADS), 0, (hipStream_t)stream, a, loss, avg);
  BEVAMD_LAUNCH_CHECK("centerhead_box_loss forward");
  return BEVAMD_OK;
}

int bevamd_centerhead_box_loss_backward(const float* const* maps, const long long* const* ind, const float* const* target,
                                        const unsigned char* const* mask, int num_tasks, int batch, int max_objs, long long hw,
                                        const float* code_weights, float loss_weight, const float* avg, const float* grad_out,
                                        float* const* grad_maps, void* stream) {
  ChArgs a;
  BEVAMD_REQUIRE(grad_maps != nullptr, "centerhead_box_loss_backward: grad_maps is a host array of 5 * tasks device pointers");
  const int rc = ch_fill(a, "centerhead_box_loss_backward", maps, ind, target, mask, num_tasks, batch, max_objs, hw, code_weights, loss_weight,
                         grad_maps);
  if (rc != BEVAMD_OK) return rc;
  BEVAMD_REQUIRE(avg != nullptr && grad_out != nullptr, "centerhead_box_loss_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const long long largest = (long long)batch * 3 * hw;
  const int chunks = (int)((largest + HL_THREADS - 1) / HL_THREADS < 256 ? (largest + HL_THREADS - 1) / HL_THREADS : 256);
  hipLaunchKernelGGL(zero_maps_kernel, dim3(chunks, 5 * num_tasks), dim3(HL_THREADS), 0, s, a);
  BEVAMD_LAUNCH_CHECK("centerhead_box_loss zero");
  hipLaunchKernelGGL(chbox_scatter_kernel, dim3(batch, num_tasks), dim3(HL_THREADS), 0, s, a, avg, grad_out);
  BEVAMD_LAUNCH_CHECK("centerhead_box_loss scatter");
  return BEVAMD_OK;
}

}  // extern "C"
