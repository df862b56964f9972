// The two non-learned ends of the TransFusion detection head, gfx950.
//
// Replaces (reference):
//   mmdet3d/models/heads/bbox/transfusion.py:239-274   sigmoid, zero tensor, max_pool2d, padded slice write, two class overwrites,
//                                                      compare, multiply and a FULL argsort of C*H*W values per sample
//   transfusion.py:275-295, 322-325                    three gathers on the proposal positions
//   transfusion.py:725-749 + TransFusionBBoxCoder.decode (core/bbox/coders/transfusion_bbox_coder.py:39-124)
//                                                      about 25 small torch ops and boolean-mask indexing per sample
//   core/post_processing/box3d_nms.py:181-219          circle_nms: a numba loop on the host behind a .cpu().numpy() round trip
//
// Native formulation:
//   * bevamd_head_proposals: (1) one pass over the logits fuses sigmoid, the k x k window maximum and the compaction of the cells
//     with a positive suppressed score into a per-sample candidate list of 64-bit keys (score bits high, complemented flat index
//     low: key order IS the defined order, so the order the atomics compact in is irrelevant); (2) one workgroup per sample finds
//     the K-th largest key with an MSB-first radix select (11-bit digits, LDS histogram), collects the K keys at or above it,
//     rank-sorts them in LDS and, when fewer than K cells survive, appends the lowest flat indices that are not candidates (they
//     all lie below 2K).  Three launches for any batch size, nothing read back.
//   * bevamd_head_gather_queries: one launch; the suppressed score at the C*K cells of a sample is recomputed from the logits with
//     the device function of (1), so its bits agree with top_score.
//   * bevamd_transfusion_decode: one thread per proposal, the reference's fp32 operation order.
//   * bevamd_circle_nms: one workgroup per segment: rank sort of the live rows by (score, lower index first) in LDS, then per block
//     of 64 sorted rows one wave resolves the block greedily on 64-bit words and every later row tests itself against the rows
//     the block kept.
// The unit is compiled with fp contract(off): products and sums round separately like the reference's separate torch / numpy ops.
// exp and atan2 are evaluated in double and rounded once (the sigmoid is monotone and within half an ulp of the exact value).
#include "common.h"
#include "head_select.h"

#include <math.h>

#pragma clang fp contract(off)

namespace bevamd {
namespace head {


// sigmoid(plane[y][x]) where it equals the maximum of its k x k window (pad = k / 2), else 0; cells closer than pad to the border
// are 0 (the reference's local_max is zero there); an exempt class keeps every cell.  The sigmoid is monotone, so the window
// maximum is taken over the logits.
__device__ __forceinline__ float he_suppressed(const float* __restrict__ plane, int y, int x, int H, int W, int pad, bool exempt) {
  const float v = plane[(size_t)y * W + x];
  if (exempt || pad == 0) return he_sigmoid(v);
  if (y < pad || y >= H - pad || x < pad || x >= W - pad) return 0.f;
  float m = v;
  for (int dy = -pad; dy <= pad; ++dy)
    for (int dx = -pad; dx <= pad; ++dx) m = fmaxf(m, plane[(size_t)(y + dy) * W + (x + dx)]);
  const float s = he_sigmoid(v);
  if (m == v) return s;
  return he_sigmoid(m) == s ? s : 0.f;   // distinct logits that saturate to one sigmoid: the reference compares the sigmoids
}

__device__ __forceinline__ bool he_exempt(unsigned long long mask, int c) { return c < 64 && ((mask >> c) & 1ull); }

// ---- (a) proposals --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void candidates_kernel(const float* __restrict__ logits, int C, int H, int W, int pad,
                                                         unsigned long long exempt, unsigned long long* __restrict__ cand,
                                                         unsigned* __restrict__ cnt) {
  const int b = blockIdx.y;
  const unsigned hw = (unsigned)H * W, chw = (unsigned)C * hw;
  const unsigned flat = blockIdx.x * 256u + threadIdx.x;
  float s = 0.f;
  if (flat < chw) {
    const int c = (int)(flat / hw);
    const unsigned r = flat - (unsigned)c * hw;
    const int y = (int)(r / W), x = (int)(r - (unsigned)y * W);
    s = he_suppressed(logits + ((size_t)b * C + c) * hw, y, x, H, W, pad, he_exempt(exempt, c));
  }
  const bool keep = s > 0.f;
  const unsigned long long m = __ballot(keep);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  unsigned base = 0;
  if (lane_id() == leader) base = atomicAdd(&cnt[b], (unsigned)__popcll(m));
  base = (unsigned)__shfl((int)base, leader, 64);
  if (keep) {
    const unsigned slot = base + (unsigned)__popcll(m & lanemask_lt());   // < chw: every cell is counted at most once
    cand[(size_t)b * chw + slot] = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(~flat);
  }
}

__device__ __forceinline__ void he_write_proposal(long long* __restrict__ top_class, long long* __restrict__ top_index,
                                                  float* __restrict__ top_score, size_t at, unsigned flat, unsigned hw, float s) {
  const unsigned c = flat / hw;
  top_class[at] = (long long)c;
  top_index[at] = (long long)(flat - c * hw);
  top_score[at] = s;
}

__global__ __launch_bounds__(HE_SEL_THREADS) void select_kernel(const unsigned long long* __restrict__ cand_all,
                                                                const unsigned* __restrict__ cnt, unsigned chw, unsigned hw, int K,
                                                                long long* __restrict__ top_class, long long* __restrict__ top_index,
                                                                float* __restrict__ top_score) {
  const int b = blockIdx.x;
  const size_t out0 = (size_t)b * K;
  he_select_segment(cand_all + (size_t)b * chw, min(cnt[b], chw), chw, K, [=](unsigned pos, unsigned long long key) {
    he_write_proposal(top_class, top_index, top_score, out0 + pos, ~(unsigned)key, hw, __uint_as_float((unsigned)(key >> 32)));
  });
}

// ---- (b) gathers at the proposals -------------------------------------------------------------------------------------------
// rows of a sample: Cf feature channels, then C heatmap classes, then the 2 position columns; K proposals per row
template <typename T>
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ logits, int C, int H, int W, int pad,
                                                     unsigned long long exempt, const long long* __restrict__ top_index, int K,
                                                     const T* __restrict__ feat, int Cf, const float* __restrict__ bev_pos,
                                                     int pos_batch, T* __restrict__ query_feat, float* __restrict__ query_pos,
                                                     float* __restrict__ query_score) {
  const int b = blockIdx.y;
  const long long total = (long long)(Cf + C + 2) * K;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int r = (int)(e / K), k = (int)(e - (long long)r * K);
  const long long hw = (long long)H * W;
  const long long idx = top_index[(size_t)b * K + k];
  const bool ok = idx >= 0 && idx < hw;   // an index outside the map reads nothing and yields 0
  if (r < Cf) {
    query_feat[((size_t)b * Cf + r) * K + k] = ok ? feat[((size_t)b * Cf + r) * hw + idx] : T(0);
  } else if (r < Cf + C) {
    const int c = r - Cf;
    float s = 0.f;
    if (ok) s = he_suppressed(logits + ((size_t)b * C + c) * hw, (int)(idx / W), (int)(idx % W), H, W, pad, he_exempt(exempt, c));
    query_score[((size_t)b * C + c) * K + k] = s;
  } else {
    const int d = r - Cf - C;
    const size_t pb = pos_batch == 1 ? 0 : (size_t)b;
    query_pos[((size_t)b * K + k) * 2 + d] = ok ? bev_pos[(pb * hw + idx) * 2 + d] : 0.f;
  }
}

// ---- (c) decode ---------------------------------------------------------------------------------------------------------------
struct DecodeConst {
  float osf, vs0, vs1, pc0, pc1;   // out_size_factor, voxel_size[:2], pc_range[:2], each rounded once to fp32
  float lo[3], hi[3];              // post_center_range
  int has_range;
  float thr;
  int use_thr;
};

__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ heat, const float* __restrict__ center,
                                                     const float* __restrict__ height, const float* __restrict__ dim,
                                                     const float* __restrict__ rot, const float* __restrict__ vel,
                                                     const float* __restrict__ qscore, const long long* __restrict__ qlabel, int B,
                                                     int C, int K, int pitch, DecodeConst dc, float* __restrict__ boxes,
                                                     float* __restrict__ scores, long long* __restrict__ labels,
                                                     unsigned char* __restrict__ valid) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= B * K) return;
  const int b = t / K, k = t - b * K;
  const size_t off = (size_t)(pitch - K) + k;   // the LAST K of `pitch` proposals
  const long long lab = qscore ? qlabel[t] : -1;

  // (sigmoid(heatmap) * query_heatmap_score * one_hot).max(1): the first class attaining the maximum.  Without query scores
  // (TransFusionBBoxCoder.decode on its own) `heat` already holds the scores.
  float best = 0.f;
  int best_c = 0;
  for (int c = 0; c < C; ++c) {
    float v = 0.f;
    if (!qscore) v = heat[((size_t)b * C + c) * pitch + off];
    else if (c == lab) v = he_sigmoid(heat[((size_t)b * C + c) * pitch + off]) * qscore[((size_t)b * C + c) * K + k];
    if (c == 0 || v > best) { best = v; best_c = c; }
  }

  const int W = vel ? 9 : 7;
  float* __restrict__ o = boxes + (size_t)t * W;
  const float cx = center[((size_t)b * 2 + 0) * pitch + off] * dc.osf * dc.vs0 + dc.pc0;
  const float cy = center[((size_t)b * 2 + 1) * pitch + off] * dc.osf * dc.vs1 + dc.pc1;
  const float d0 = (float)exp((double)dim[((size_t)b * 3 + 0) * pitch + off]);
  const float d1 = (float)exp((double)dim[((size_t)b * 3 + 1) * pitch + off]);
  const float d2 = (float)exp((double)dim[((size_t)b * 3 + 2) * pitch + off]);
  const float z = height[(size_t)b * pitch + off] - d2 * 0.5f;   // gravity centre to bottom centre
  const float yaw = (float)atan2((double)rot[((size_t)b * 2 + 0) * pitch + off], (double)rot[((size_t)b * 2 + 1) * pitch + off]);
  o[0] = cx; o[1] = cy; o[2] = z; o[3] = d0; o[4] = d1; o[5] = d2; o[6] = yaw;
  if (vel) {
    o[7] = vel[((size_t)b * 2 + 0) * pitch + off];
    o[8] = vel[((size_t)b * 2 + 1) * pitch + off];
  }
  scores[t] = best;
  labels[t] = best_c;
  bool ok = true;
  if (dc.has_range)
    ok = cx >= dc.lo[0] && cy >= dc.lo[1] && z >= dc.lo[2] && cx <= dc.hi[0] && cy <= dc.hi[1] && z <= dc.hi[2];
  if (dc.use_thr) ok = ok && best > dc.thr;
  valid[t] = ok ? 1 : 0;
}

// ---- (d) circle NMS -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HE_MAX_K) void circle_nms_kernel(const float* __restrict__ xy, const float* __restrict__ score,
                                                              const int* __restrict__ seg_off, const float* __restrict__ seg_thr,
                                                              const unsigned char* __restrict__ live, int N, int max_rows, int pms,
                                                              unsigned char* __restrict__ keep, long long* __restrict__ order,
                                                              int* __restrict__ counts) {
  __shared__ unsigned long long skey[HE_MAX_K];
  __shared__ float sx[HE_MAX_K], sy[HE_MAX_K];
  __shared__ short sid[HE_MAX_K];            // sorted position -> row of the segment
  __shared__ unsigned char kflag[HE_MAX_K];  // row of the segment -> kept
  __shared__ unsigned long long kept_w[HE_MAX_K / 64];

  const int tid = threadIdx.x, lane = tid & 63;
  const int s = blockIdx.x;
  const int beg = max(seg_off[s], 0), end = min(seg_off[s + 1], N);
  const int n = end - beg;
  if (n <= 0) {
    if (tid == 0) counts[s] = 0;
    return;
  }
  if (n > max_rows) {   // longer than the caller's bound: nothing kept, count -1
    for (int i = tid; i < n; i += HE_MAX_K) keep[beg + i] = 0;
    if (tid == 0) counts[s] = -1;
    return;
  }

  // descending (score, lower row first) as one 64-bit key; 0: not live
  unsigned long long mine = 0;
  if (tid < n && (!live || live[beg + tid])) {
    unsigned bits = __float_as_uint(score[beg + tid]);
    bits = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    mine = ((unsigned long long)bits << 32) | (unsigned long long)(~(unsigned)tid);
  }
  skey[tid] = mine;
  kflag[tid] = 0;
  if (tid < HE_MAX_K / 64) kept_w[tid] = 0;
  const int m = __syncthreads_count(mine != 0);
  if (mine) {
    int r = 0;
    for (int j = 0; j < n; ++j) r += skey[j] > mine ? 1 : 0;
    sx[r] = xy[(size_t)(beg + tid) * 2];
    sy[r] = xy[(size_t)(beg + tid) * 2 + 1];
    sid[r] = (short)tid;
  }
  __syncthreads();

  const float thr = seg_thr[s];
  if (!(thr > 0.f)) {   // transfusion.py:823-824: every live row, no cap
    if (tid < n) keep[beg + tid] = mine ? 1 : 0;
    if (order && tid < m) order[beg + tid] = (long long)beg + sid[tid];
    if (tid == 0) counts[s] = m;
    return;
  }

  const float x = tid < m ? sx[tid] : 0.f, y = tid < m ? sy[tid] : 0.f;
  bool sup = false;
  int total = 0;
  const int nblk = (m + 63) >> 6;
  for (int rb = 0; rb < nblk; ++rb) {
    if ((tid >> 6) == rb) {
      const int base = rb * 64;
      unsigned long long diag = 0;   // earlier rows of this block within the radius of mine
      if (tid < m)
        for (int j = 0; j < lane; ++j) {
          const float dx = sx[base + j] - x, dy = sy[base + j] - y;
          if (dx * dx + dy * dy <= thr) diag |= 1ull << j;
        }
      const bool can = tid < m && !sup;
      unsigned long long kept = 0;
      for (int t = 0; t < 64; ++t) {
        const int mine_kept = (can && (diag & kept) == 0ull) ? 1 : 0;
        if (__shfl(mine_kept, t, 64)) kept |= 1ull << t;
      }
      if (lane == 0) kept_w[rb] = kept;
    }
    __syncthreads();
    unsigned long long k = kept_w[rb];
    total += __popcll(k);
    if (total >= pms) break;   // block-uniform: later rows are cut by post_max_size
    if (tid < m && (tid >> 6) > rb && !sup)
      while (k) {
        const int i = rb * 64 + __ffsll((long long)k) - 1;
        k &= k - 1;
        const float dx = sx[i] - x, dy = sy[i] - y;
        if (dx * dx + dy * dy <= thr) {
          sup = true;
          break;
        }
      }
  }

  if (tid < m) {
    const unsigned long long w = kept_w[tid >> 6];
    if ((w >> lane) & 1ull) {
      int rank = __popcll(w & lanemask_lt());
      for (int q = 0; q < (tid >> 6); ++q) rank += __popcll(kept_w[q]);
      if (rank < pms) {
        kflag[sid[tid]] = 1;
        if (order) order[beg + rank] = (long long)beg + sid[tid];
      }
    }
  }
  __syncthreads();
  if (tid < n) keep[beg + tid] = kflag[tid];
  if (tid == 0) counts[s] = min(total, pms);
}

}  // namespace head
}  // namespace bevamd

using namespace bevamd;
using namespace bevamd::head;

static int he_check_map(const char* what, int B, int C, int H, int W, int k, int K) {
  BEVAMD_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && B <= 65535 && (long long)C * H * W <= 0x7fffffffLL,
                 "%s: bad sizes (B %d, C %d, %d x %d)", what, B, C, H, W);
  BEVAMD_REQUIRE(k >= 1 && (k & 1) && k <= H && k <= W, "%s: kernel size %d (odd, at most %d x %d)", what, k, H, W);
  BEVAMD_REQUIRE(K >= 1 && K <= HE_MAX_K && (long long)K <= (long long)C * H * W,
                 "%s: num_proposals %d (1 .. %d, at most C*H*W)", what, K, HE_MAX_K);
  return BEVAMD_OK;
}

extern "C" {

size_t bevamd_head_proposals_workspace_bytes(int batch, int classes, int height, int width) {
  if (batch < 1 || classes < 1 || height < 1 || width < 1 || (long long)classes * height * width > 0x7fffffffLL) return 0;
  return align_up((size_t)batch * classes * height * width * 8, 256) + align_up((size_t)batch * 4, 256);
}

int bevamd_head_proposals(const float* logits, int batch, int classes, int height, int width, int kernel_size,
                          unsigned long long exempt_mask, int num_proposals, long long* top_class, long long* top_index,
                          float* top_score, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = he_check_map("head_proposals", batch, classes, height, width, kernel_size, num_proposals);
  if (rc) return rc;
  BEVAMD_REQUIRE(logits && top_class && top_index && top_score, "head_proposals: null buffer");
  if (!ws || ws_bytes < bevamd_head_proposals_workspace_bytes(batch, classes, height, width)) {
    set_error("head_proposals: workspace too small");
    return BEVAMD_ERR_WORKSPACE;
  }
  const unsigned hw = (unsigned)height * width, chw = (unsigned)classes * hw;
  Carver cv(ws, ws_bytes);
  unsigned long long* cand = cv.take<unsigned long long>((size_t)batch * chw);
  unsigned* cnt = cv.take<unsigned>((size_t)batch);
  rc = device_fill_u32(cnt, (size_t)batch, 0u, stream);
  if (rc) return rc;
  candidates_kernel<<<dim3(cdiv(chw, 256), batch), dim3(256), 0, stream>>>(logits, classes, height, width, kernel_size / 2,
                                                                          exempt_mask, cand, cnt);
  BEVAMD_LAUNCH_CHECK("head_candidates");
  select_kernel<<<dim3(batch), dim3(HE_SEL_THREADS), 0, stream>>>(cand, cnt, chw, hw, num_proposals, top_class, top_index, top_score);
  BEVAMD_LAUNCH_CHECK("head_select");
  return BEVAMD_OK;
}

int bevamd_head_gather_queries(const float* logits, int batch, int classes, int height, int width, int kernel_size,
                               unsigned long long exempt_mask, const long long* top_index, int num_proposals, const void* feat,
                               int feat_dtype, int feat_channels, const float* bev_pos, int bev_pos_batch, void* query_feat,
                               float* query_pos, float* query_heatmap_score, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = he_check_map("head_gather_queries", batch, classes, height, width, kernel_size, num_proposals);
  if (rc) return rc;
  BEVAMD_REQUIRE(feat_dtype == 0 || feat_dtype == 1, "head_gather_queries: feat_dtype %d (0 fp32, 1 fp16)", feat_dtype);
  BEVAMD_REQUIRE(feat_channels >= 1 && (bev_pos_batch == 1 || bev_pos_batch == batch),
                 "head_gather_queries: bad sizes (Cf %d, bev_pos batch %d of %d)", feat_channels, bev_pos_batch, batch);
  BEVAMD_REQUIRE(logits && top_index && feat && bev_pos && query_feat && query_pos && query_heatmap_score,
                 "head_gather_queries: null buffer");
  const dim3 grid(cdiv((long long)(feat_channels + classes + 2) * num_proposals, 256), batch);
  if (feat_dtype == 0)
    gather_kernel<float><<<grid, dim3(256), 0, stream>>>(logits, classes, height, width, kernel_size / 2, exempt_mask, top_index,
                                                         num_proposals, (const float*)feat, feat_channels, bev_pos, bev_pos_batch,
                                                         (float*)query_feat, query_pos, query_heatmap_score);
  else
    gather_kernel<_Float16><<<grid, dim3(256), 0, stream>>>(logits, classes, height, width, kernel_size / 2, exempt_mask, top_index,
                                                            num_proposals, (const _Float16*)feat, feat_channels, bev_pos,
                                                            bev_pos_batch, (_Float16*)query_feat, query_pos, query_heatmap_score);
  BEVAMD_LAUNCH_CHECK("head_gather_queries");
  return BEVAMD_OK;
}

int bevamd_transfusion_decode(const float* heatmap, const float* center, const float* height, const float* dim, const float* rot,
                              const float* vel, const float* query_heatmap_score, const long long* query_labels, int batch,
                              int classes, int num_proposals, int pitch, const float* coder, const float* post_center_range,
                              float score_threshold, int use_score_threshold, float* boxes, float* scores, long long* labels,
                              unsigned char* valid, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(batch >= 1 && classes >= 1 && num_proposals >= 1 && pitch >= num_proposals &&
                     (long long)batch * pitch * (classes > 3 ? classes : 3) <= 0x7fffffffLL,
                 "transfusion_decode: bad sizes (B %d, C %d, K %d of %d)", batch, classes, num_proposals, pitch);
  BEVAMD_REQUIRE(coder != nullptr, "transfusion_decode: coder constants are null");
  BEVAMD_REQUIRE(heatmap && center && height && dim && rot && boxes && scores && labels && valid, "transfusion_decode: null buffer");
  BEVAMD_REQUIRE((query_heatmap_score == nullptr) == (query_labels == nullptr),
                 "transfusion_decode: query_heatmap_score and query_labels come together");
  DecodeConst dc;
  dc.osf = coder[0]; dc.vs0 = coder[1]; dc.vs1 = coder[2]; dc.pc0 = coder[3]; dc.pc1 = coder[4];
  dc.has_range = post_center_range ? 1 : 0;
  for (int d = 0; d < 3; ++d) {
    dc.lo[d] = post_center_range ? post_center_range[d] : 0.f;
    dc.hi[d] = post_center_range ? post_center_range[3 + d] : 0.f;
  }
  dc.thr = score_threshold;
  dc.use_thr = use_score_threshold ? 1 : 0;
  decode_kernel<<<dim3(cdiv((long long)batch * num_proposals, 256)), dim3(256), 0, stream>>>(
      heatmap, center, height, dim, rot, vel, query_heatmap_score, query_labels, batch, classes, num_proposals, pitch, dc, boxes,
      scores, labels, valid);
  BEVAMD_LAUNCH_CHECK("transfusion_decode");
  return BEVAMD_OK;
}

int bevamd_circle_nms(const float* xy, const float* score, int num_rows, const int* seg_offsets, int num_segments,
                      const float* seg_thresh, int max_segment_rows, int post_max_size, const unsigned char* live,
                      unsigned char* keep, long long* keep_order, int* seg_counts, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BEVAMD_REQUIRE(num_rows >= 0 && num_segments >= 0 && max_segment_rows >= 0 && post_max_size >= 0,
                 "circle_nms: bad sizes (N %d, S %d, rows per segment %d, post_max_size %d)", num_rows, num_segments,
                 max_segment_rows, post_max_size);
  if (max_segment_rows > HE_MAX_K) {
    set_error("circle_nms: not supported (segments of up to %d rows, at most %d)", max_segment_rows, HE_MAX_K);
    return BEVAMD_ERR_UNSUPPORTED;
  }
  if (num_segments == 0) return BEVAMD_OK;
  BEVAMD_REQUIRE(seg_offsets && seg_thresh && seg_counts, "circle_nms: null segment table");
  BEVAMD_REQUIRE(num_rows == 0 || (xy && score && keep), "circle_nms: null buffer");
  circle_nms_kernel<<<dim3(num_segments), dim3(HE_MAX_K), 0, stream>>>(xy, score, seg_offsets, seg_thresh, live, num_rows,
                                                                      max_segment_rows, post_max_size, keep, keep_order, seg_counts);
  BEVAMD_LAUNCH_CHECK("circle_nms");
  return BEVAMD_OK;
}

}  // extern "C"
