/* C ABI of the OPTIONAL library libbevfusion_amd_ext.so: the exports of the reference's pybind modules that lie OUTSIDE the hot
 * path of SURVEY.md §8 (sparse max pooling of sparse_conv_ext, dynamic scatter of voxel_layer).  They were built after the hot
 * path met its bar and live in their own library (bevfusion_amd/csrc/ext/), so that libbevfusion_amd.so carries only what the
 * path runs; the ext library links against it for the shared primitives (scan, sort, error string).  Same conventions as
 * bevfusion_amd.h. */
#ifndef BEVFUSION_AMD_EXT_H_
#define BEVFUSION_AMD_EXT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Dynamic scatter.  Replace voxel_layer.dynamic_point_to_voxel_forward / _backward
 *   (voxel/src/voxelization.cpp:6-11 -> voxelization.h:108-140 -> scatter_points_cuda.cu:197-330).
 * bevamd_dynamic_scatter_index: coors [num_points, ndim] int32 (ndim 1..4); rows with a negative entry are dropped.
 *   out_coors [num_points, ndim] receives the distinct rows in ascending lexicographic order (what
 *   at::unique_dim(sorted) yields), coors_map [num_points] the voxel of every point (-1 for dropped points),
 *   reduce_count [num_points] the points per voxel; order [num_points] (sorted position -> point id; points of a voxel
 *   are consecutive, ascending point id) and seg_start [num_points + 1] (first sorted position of every voxel, then
 *   the number of kept points) feed bevamd_dynamic_scatter_reduce.  Only the first *num_voxels rows of the per-voxel
 *   arrays are written.  num_voxels_dev [1] always receives the count; num_voxels_host (optional) makes the call
 *   synchronise and return it.  (The call reads the column maxima back once to size its sort keys.)
 * bevamd_dynamic_scatter_reduce: reduced [num_voxels, num_feats] = sum / mean / max (reduce_type 0 / 1 / 2, the
 *   reference's reduce_t) of feats [num_points, num_feats] fp32 over each voxel's points, in ascending point order —
 *   no float atomics, bit-reproducible (the reference's atomicAdd order is not).
 * bevamd_dynamic_scatter_backward: grad_feats [num_points, num_feats] from grad_reduced [num_voxels, num_feats]:
 *   sum: g[voxel]; mean: g[voxel] / count; max: the lowest-numbered point attaining the maximum takes g, the others 0
 *   (reduce_from_ws: int32 [num_voxels * num_feats] scratch, max only; feats / reduced may be NULL otherwise). */
size_t bevamd_dynamic_scatter_workspace_bytes(int num_points);
int bevamd_dynamic_scatter_index(const int* coors, int num_points, int ndim, int* out_coors, int* coors_map,
                                 int* reduce_count, int* order, int* seg_start, int* num_voxels_dev,
                                 int* num_voxels_host, void* ws, size_t ws_bytes, void* stream);
int bevamd_dynamic_scatter_reduce(const float* feats, int num_feats, const int* order, const int* seg_start,
                                  int num_voxels, int reduce_type, float* reduced, void* stream);
int bevamd_dynamic_scatter_backward(float* grad_feats, const float* grad_reduced, const float* feats,
                                    const float* reduced, const int* coors_map, const int* reduce_count,
                                    int num_points, int num_voxels, int num_feats, int reduce_type,
                                    int* reduce_from_ws, void* stream);


/* Sparse max pooling.  Replace sparse_conv_ext.indice_maxpool_{fp32,half} and indice_maxpool_backward_{fp32,half}
 *   (spconv/src/all.cc:39-46 -> pool_ops.h:25-97 indiceMaxPool / indiceMaxPoolBackward; arithmetic of
 *    maxpool_cpu.cc:22-66).
 * forward : out[o][c] = max(0, max over offsets k with nbr[k][o] >= 0 of features[nbr[k][o]][c]) — the reference's
 *           output starts from zeros and only takes strictly larger inputs.  features [num_in, feat_stride],
 *           out [num_out, out_stride] (strides in elements, >= channels).
 * backward: in_grad[i][c] = sum over offsets k (ascending) with o = nbr_t[k][i] >= 0 and
 *           out_features[o][c] == features[i][c] of out_grad[o][c]; all four tensors contiguous [rows, channels];
 *           nbr_t is the input-stationary table (bevamd_spconv_transpose_nbr / nbr_from_pairs with inverse = 1).
 * dtype: 0 fp32, 1 fp16, 2 bf16.  One launch each, no atomics, results bit-reproducible. */
int bevamd_spconv_maxpool_forward(const void* features, int dtype, int feat_stride, const int* nbr, int nbr_stride,
                                  int num_out, int kernel_volume, int channels, void* out, int out_stride,
                                  void* stream);
int bevamd_spconv_maxpool_backward(const void* features, const void* out_features, const void* out_grad, int dtype,
                                   const int* nbr_t, int nbr_t_stride, int num_in, int kernel_volume, int channels,
                                   void* in_grad, void* stream);


/* Pillar / radar encoders.  Replace PillarFeatureNet / RadarFeatureNet / PointPillarsScatter of
 *   mmdet3d/models/backbones/pillar_encoder.py and radar_encoder.py.
 * Common inputs: voxels [num_pillars, max_points, num_features] fp32, num_points [num_pillars] int32, coors [num_pillars, 4]
 *   int32 ordered (b, x, y, z); mode 0 = pillar, 1 = radar; geom: HOST array of 10 floats
 *   {vx, vy, x_offset, y_offset, lo_x, lo_y, lo_z, hi_x - lo_x, hi_y - lo_y, hi_z - lo_z}, each computed in double the way
 *   the reference's constructor does and rounded once to fp32.
 * bevamd_pillar_decorate: out [num_pillars, max_points, F_out].
 *   pillar: F_out = F + 5 (+ 1 with_distance): [features, xyz - sum_over_P(xyz) / num_points, x - (float(cx) * vx + x_offset),
 *           y - (float(cy) * vy + y_offset), (|xyz|)]; every row p >= num_points is multiplied by 0.
 *   radar : F_out = F + 2: [features with xyz replaced by (v - lo) / (hi - lo), f_center from the un-normalised x, y]; the same
 *           mask, then nan_to_num (NaN -> 0, +-inf -> +-FLT_MAX).  with_distance is ignored.
 *   No FMA contraction: every column but f_cluster is bit-equal to the reference's fp32 arithmetic.
 * bevamd_pillar_stack_forward: the eval-mode network in one launch: decorate, then per layer l Linear without bias
 *   (weights[l]: DEVICE [K_l, units_l] fp32 — the Linear weight TRANSPOSED) -> folded BatchNorm (scales[l], shifts[l]: DEVICE
 *   [units_l]) -> ReLU -> combine: pillar non-last [x, max_over_P(x)], radar non-last x, last max_over_P(x); out
 *   [num_pillars, units_last] fp32.  The max runs over all P rows: the padded rows (all equal) are computed once per pillar.
 *   units / weights / scales / shifts are HOST arrays of num_layers entries.  Limits: at most 4 layers, units multiples of 4 up
 *   to 128 (pillar non-last: up to 64), num_features up to 64, max_points up to 32; anything else returns 4 (unsupported)
 *   before any GPU work.  num_points is clamped to [0, max_points] for the row count.
 * bevamd_pillar_scatter_forward: canvas [batch_size, channels, nx, ny] (dtype 0 fp32, 1 fp16) with
 *   canvas[b, c, x * ny + y] = feats[row, c], zero elsewhere; the whole canvas is written.  winner: int32
 *   [batch_size, nx * ny] scratch that the call resets itself and leaves holding the winning row of every cell (-1: empty) for
 *   the backward.  Duplicated cells: the highest row wins; rows with b outside [0, batch_size) or x / y outside the canvas
 *   are dropped.
 * bevamd_pillar_scatter_backward: grad_feats [num_pillars, channels] = grad_canvas[b, :, cell] for the winner of a cell, 0 for
 *   every other row.
 * No device synchronisation, no float atomics: results are bit-reproducible. */
int bevamd_pillar_decorate(const float* voxels, const int* num_points, const int* coors, int num_pillars, int max_points,
                           int num_features, int mode, int with_distance, const float* geom, float* out, void* stream);
int bevamd_pillar_stack_forward(const float* voxels, const int* num_points, const int* coors, int num_pillars,
                                int max_points, int num_features, int mode, int with_distance, const float* geom,
                                int num_layers, const int* units, const void* const* weights, const void* const* scales,
                                const void* const* shifts, float* out, void* stream);
int bevamd_pillar_scatter_forward(const void* feats, int dtype, const int* coors, int num_pillars, int channels,
                                  int batch_size, int nx, int ny, int* winner, void* canvas, void* stream);
int bevamd_pillar_scatter_backward(const void* grad_canvas, int dtype, const int* coors, const int* winner,
                                   int num_pillars, int channels, int batch_size, int nx, int ny, void* grad_feats,
                                   void* stream);


/* The two non-learned ends of TransFusionHead.  Nothing below synchronises the device or reads anything back; every call is a
 * fixed, small number of launches on `stream` and can be captured in a graph.  All heatmap inputs must be FINITE.
 *
 * bevamd_head_proposals: replaces mmdet3d/models/heads/bbox/transfusion.py:239-274 (sigmoid, max_pool2d into a zero-padded
 *   local_max, the two class overwrites, compare, multiply, full argsort).  logits [batch, classes, height, width] fp32, FINITE.
 *   s = sigmoid(x); for a class whose bit is clear in exempt_mask, s is kept only where it equals the maximum of its
 *   kernel_size x kernel_size window (odd, <= height and width) and is 0 closer than kernel_size / 2 to the border; classes
 *   >= 64 are never exempt.  The proposals are the num_proposals (1 .. 1024, <= classes * height * width) largest of the
 *   classes * height * width values of a sample in STABLE descending order: equal values — ties, and the zeros that fill the
 *   list when fewer cells survive — come in ascending flat index c * height * width + y * width + x (the reference's argsort
 *   leaves that order open).  top_class, top_index (position in height * width) [batch, num_proposals] int64, top_score fp32.
 *   No sort of the map: candidates are compacted, an MSB radix select finds the K-th key, one workgroup per sample sorts K keys.
 *   ws: bevamd_head_proposals_workspace_bytes (0 for sizes the call rejects); it needs no initialisation.
 * bevamd_head_gather_queries: replaces transfusion.py:275-295 and :322-325.  query_feat [batch, feat_channels, num_proposals]
 *   from feat [batch, feat_channels, height * width] (feat_dtype 0 fp32, 1 fp16); query_pos [batch, num_proposals, 2] from
 *   bev_pos [bev_pos_batch = 1 or batch, height * width, 2]; query_heatmap_score [batch, classes, num_proposals]: the suppressed
 *   sigmoid of EVERY class at each proposal's position, recomputed from the logits by the function bevamd_head_proposals uses
 *   (same bits as top_score).  A top_index outside [0, height * width) reads nothing and yields zeros.
 * bevamd_transfusion_decode: replaces transfusion.py:725-749 and TransFusionBBoxCoder.decode(filter=True)
 *   (mmdet3d/core/bbox/coders/transfusion_bbox_coder.py:39-124).  heatmap [batch, classes, pitch] logits, center [batch, 2, pitch],
 *   height [batch, 1, pitch], dim [batch, 3, pitch], rot [batch, 2, pitch], vel [batch, 2, pitch] or NULL: the LAST num_proposals
 *   of the pitch columns are decoded; query_heatmap_score [batch, classes, num_proposals], query_labels [batch, num_proposals]
 *   int64.  coder: HOST {out_size_factor, voxel_size[0], voxel_size[1], pc_range[0], pc_range[1]} as fp32;
 *   post_center_range: HOST 6 floats or NULL (no range test).  boxes [batch, num_proposals, 7 or 9 with vel] =
 *   (x * osf * vs + pc, y likewise, height - exp(dim2) * 0.5, exp(dim), atan2(rot0, rot1), vel) in the reference's fp32 operation
 *   order without FMA contraction (centre and velocity columns are bit-equal to the reference's CPU result; exp / atan2 are
 *   rounded once from double); scores = max over classes of sigmoid(heatmap) * query_heatmap_score * one_hot(query_labels),
 *   labels the first class attaining it (query_heatmap_score and query_labels both NULL: heatmap already holds the scores, as
 *   in TransFusionBBoxCoder.decode called on its own, and pitch columns of it are read likewise); valid uint8 = inside post_center_range on the first three columns AND
 *   (use_score_threshold == 0 OR score > score_threshold) — the reference skips the score test for a falsy threshold, so the
 *   caller passes use_score_threshold = 0 for 0.0.  The inputs are NOT modified (the reference overwrites center and dim).
 * bevamd_circle_nms: replaces circle_nms of mmdet3d/core/post_processing/box3d_nms.py:181-219, segmented.  xy [num_rows, 2],
 *   score [num_rows], seg_offsets [num_segments + 1] int32 (device), seg_thresh [num_segments] fp32 (device), live: optional uint8
 *   [num_rows] (0 rows take no part).  Per segment: greedy in descending score (equal scores: lower row first); row j is dropped
 *   when a kept row i has (xi - xj)^2 + (yi - yj)^2 <= thresh in fp32 — the threshold meets the SQUARED distance, as in the
 *   reference; only the first post_max_size kept rows stay.  A threshold <= 0 keeps every live row of the segment without the
 *   cap (transfusion.py:823-824).  keep [num_rows] uint8; keep_order (optional) [num_rows] int64: the kept rows of segment s in
 *   descending score order at seg_offsets[s] ...; seg_counts [num_segments] int32.  max_segment_rows: the caller's bound on a
 *   segment's length, at most 1024 (more: 4, unsupported, before any GPU work); a segment longer than the bound keeps nothing
 *   and reports -1.  No workspace. */
size_t bevamd_head_proposals_workspace_bytes(int batch, int classes, int height, int width);
int bevamd_head_proposals(const float* logits, int batch, int classes, int height, int width, int kernel_size,
                          unsigned long long exempt_mask, int num_proposals, long long* top_class, long long* top_index,
                          float* top_score, void* ws, size_t ws_bytes, void* stream);
int bevamd_head_gather_queries(const float* logits, int batch, int classes, int height, int width, int kernel_size,
                               unsigned long long exempt_mask, const long long* top_index, int num_proposals, const void* feat,
                               int feat_dtype, int feat_channels, const float* bev_pos, int bev_pos_batch, void* query_feat,
                               float* query_pos, float* query_heatmap_score, void* stream);
int bevamd_transfusion_decode(const float* heatmap, const float* center, const float* height, const float* dim,
                              const float* rot, const float* vel, const float* query_heatmap_score,
                              const long long* query_labels, int batch, int classes, int num_proposals, int pitch,
                              const float* coder, const float* post_center_range, float score_threshold,
                              int use_score_threshold, float* boxes, float* scores, long long* labels, unsigned char* valid,
                              void* stream);
int bevamd_circle_nms(const float* xy, const float* score, int num_rows, const int* seg_offsets, int num_segments,
                      const float* seg_thresh, int max_segment_rows, int post_max_size, const unsigned char* live,
                      unsigned char* keep, long long* keep_order, int* seg_counts, void* stream);


/* The learned ends of TransFusionHead.forward_single around the decoder layer (mmdet3d/models/heads/bbox/transfusion.py:283-288
 * and :311-312, FFN of mmdet3d/models/utils/transformer.py:496-575).  One launch each, no workspace, no device synchronisation,
 * no float atomics: equal calls give bit-equal results and both can be captured in a graph.
 *
 * bevamd_head_class_encoding: query_feat [batch, channels, num_queries] fp32, IN PLACE:
 *   query_feat[b, c, k] += weight[c, labels[b, k]] + bias[c], with labels [batch, num_queries] int64, weight
 *   [channels, num_classes] (the Conv1d weight [channels, num_classes, 1]) and bias [channels] fp32.  The sum in parentheses is
 *   rounded first, as the reference's convolution over the one-hot rounds it (its other products are exact zeros); no FMA
 *   contraction: the result is bit-equal to the reference's fp32 arithmetic.  A label outside [0, num_classes) — where
 *   F.one_hot raises — adds NOTHING to that query (not the bias either), reads nothing outside weight and raises no fault.
 *   Exactly batch * channels * num_queries floats of query_feat are read and written, batch * num_queries labels read.
 * bevamd_head_ffn_forward: every prediction head of one decoder layer in eval mode.  x [batch, in_channels, num_queries] fp32.
 *   head_channels / w1 / scales / shifts / w2 / biases / outs are HOST arrays of num_heads entries; per head h the DEVICE
 *   pointers w1[h] [head_conv, in_channels] (the first Conv1d, no bias), scales[h] / shifts[h] [head_conv] (BatchNorm1d folded:
 *   scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale), w2[h] [head_channels[h], head_conv] and
 *   biases[h] [head_channels[h]] (the second Conv1d), all fp32, w1[h] and w2[h] 16-byte aligned:
 *     out_h[b, c, col_offset + p] = biases[h][c] + sum_j w2[h][c, j] * relu(scales[h][j] * sum_k w1[h][j, k] * x[b, k, p] + shifts[h][j])
 *   with outs[h] laid out [batch, head_channels[h], out_stride]: exactly the columns [col_offset, col_offset + num_queries) of
 *   every row are written and nothing else, so layer l of an auxiliary head writes with col_offset = l * num_queries into the
 *   [batch, c, layers * num_queries] tensor the reference builds with torch.cat.  query_pos: optional [batch, num_queries, 2]
 *   fp32; with it, head center_head (2 channels; negative: none) gets + query_pos[b, p, c] after its bias, the reference's
 *   res_layer["center"] + query_pos.permute(0, 2, 1).  fp32 FMA with fp32 accumulation in ascending k and j; the hidden
 *   activations stay in LDS.  Limits, checked on the host before any GPU work, anything else returns 4 (unsupported):
 *   in_channels a multiple of 4 up to 256, head_conv a multiple of 16 up to 128, head_channels 1 .. 32, 1 .. 8 heads,
 *   num_queries >= 1, 0 <= col_offset and col_offset + num_queries <= out_stride.  batch 0 .. 65535 (0: nothing to do). */
int bevamd_head_class_encoding(float* query_feat, const long long* labels, const float* weight, const float* bias, int batch,
                               int channels, int num_queries, int num_classes, void* stream);
int bevamd_head_ffn_forward(const float* x, int batch, int in_channels, int num_queries, int head_conv, int num_heads,
                            const int* head_channels, const void* const* w1, const void* const* scales,
                            const void* const* shifts, const void* const* w2, const void* const* biases, const float* query_pos,
                            int center_head, void* const* outs, int out_stride, int col_offset, void* stream);


/* The task heads of CenterHead.forward_single in eval mode (mmdet3d/models/heads/bbox/centerpoint.py:121-125 and :351-352): for
 * every head of every task Conv2d(64 -> 64, k x k, padding k / 2, no bias) -> BatchNorm2d (folded) -> ReLU -> Conv2d(64 -> c, k x k,
 * padding k / 2, bias) on the shared map, ONE launch, no workspace, no device synchronisation, no atomics: equal calls give
 * bit-equal results, a sample's result does not depend on the batch, and the call can be captured in a graph.
 *
 * bevamd_center_heads_forward: x [batch, channels, height, width] fp32, contiguous.  heads_per_task [num_tasks] and head_channels
 *   [sum of heads_per_task] are HOST arrays (heads in task order).  packed: ONE DEVICE buffer, 16-byte aligned, of exactly
 *   packed_floats floats holding per head, heads in order, with k2 = final_kernel^2:
 *     w1 in fragment order, 4096 k2 floats: element [m][s4][lane][q] (m < 2, s4 < 8 k2, lane < 64, q < 4) is
 *       weight1[m * 32 + (lane & 31)][ci][tap / final_kernel][tap % final_kernel] with 2 * (4 * s4 + q) + (lane >> 5) = tap * 64 + ci;
 *     scale [64], shift [64]: scale = bn.weight / sqrt(running_var + eps), shift = bn.bias - running_mean * scale;
 *     w2 [c][tap][64] = weight2[c][j][tap / final_kernel][tap % final_kernel]; bias [c], padded with zeros to a multiple of 4.
 *   out: ONE buffer of exactly out_floats = batch * sum(c) * height * width floats in which head i owns the contiguous block
 *   [batch, c_i, height, width] after the blocks of the heads before it.  Every element of out is written, nothing else is, and x
 *   is only read.
 *     hidden_h[b, j, y, x] = relu(scale_h[j] * sum_{tap, ci} weight1_h[j, ci, tap] * x[b, ci, (y, x) + tap] + shift_h[j])
 *     out_h[b, c, y, x]    = bias_h[c] + sum_{tap, j} weight2_h[c, j, tap] * hidden_h[b, j, (y, x) + tap]
 *   with x and hidden taken as zero outside the map.  The first sum is four v_mfma_f32_32x32x2_f32 chains in ascending (tap, ci),
 *   chain q taking the channel pairs with (ci / 2) mod 4 = q, added as (s0 + s1) + (s2 + s3); the second is four fp32 fmaf chains in
 *   ascending (tap, j), chain q taking j mod 4 = q, added the same way; the hidden activations stay in LDS.
 *   Limits, checked on the host before any GPU work, anything else returns 4 (unsupported): channels = head_conv = 64,
 *   final_kernel 1 or 3, 1 .. 8 tasks of 1 .. 8 heads, 1 .. 16 channels per head.  height, width >= 1; batch 0 .. 65535 (0:
 *   nothing to do).  Code 1: a null pointer, bad sizes, packed_floats or out_floats that do not fit the heads. */
int bevamd_center_heads_forward(const float* x, int batch, int channels, int head_conv, int height, int width, int final_kernel,
                                int num_tasks, const int* heads_per_task, const int* head_channels, const float* packed,
                                long long packed_floats, float* out, long long out_floats, void* stream);


/* One layer of the dense BEV trunk in eval mode (mmdet3d/models/fusers/conv.py ConvFuser, models/backbones/second.py SECOND,
 * models/necks/second.py SECONDFPN): convolution + folded BatchNorm + ReLU in ONE launch on 16-bit storage (dtype 0: fp16, 1: bf16)
 * with fp32 accumulation on v_mfma_f32_16x16x32; no workspace, no device synchronisation, no atomics, no split-K: equal calls give
 * bit-equal results, a sample's result does not depend on the batch, and the call can be captured in a graph.
 *
 * bevamd_bev_conv_forward: the input is the channel concatenation of src0 (channels0) and, when channels1 > 0, src1 (channels1),
 *   both [batch, c, height, width] in src_layout (0: NCHW, 1: NHWC = [batch, height, width, c]), contiguous; an NHWC source is
 *   16-byte aligned.  Modes: mode 0 kernel 3 stride 1 or 2 (padding 1, output (H + 2 - 3) / stride + 1), mode 0 kernel 1 stride 1,
 *   mode 1 kernel 2 stride 2 (ConvTranspose2d, output 2H x 2W).  With Cin = channels0 + channels1, nch = ceil(Cin / 32),
 *   taps = kernel^2 for mode 0 and 1 for mode 1, groups = 1 for mode 0 and 4 for mode 1, packed holds exactly
 *   packed_elems = groups * out_channels * nch * taps * 32 16-bit elements, 16-byte aligned, in A-fragment order:
 *     element [g][mt][chunk][tap][lane][j] (mt < out_channels / 16, lane < 64, j < 8) is
 *     w[co = 16 mt + (lane & 15)][ci = 32 chunk + 8 (lane >> 4) + j] of tap (ky, kx) = (tap / kernel, tap % kernel) for mode 0
 *     (w = Conv2d.weight[co][ci][ky][kx]) and of tap (dy, dx) = (g / 2, g % 2) for mode 1 (w = ConvTranspose2d.weight[ci][co][dy][dx]),
 *     zero where ci >= Cin.
 *   scale, shift: [out_channels] fp32, 16-byte aligned (scale = bn.weight / sqrt(running_var + eps), shift = bn.bias -
 *   running_mean * scale; never folded into the 16-bit weights).
 *     y[b, co, p] = round16(max(fma(sum_{chunk, tap, ci} w * x, scale[co], shift[co]), 0))
 *   with x zero outside the map, ONE fp32 accumulator chain per element in ascending (chunk, tap, ci).  y is written into the
 *   channels [dst_channel_offset, dst_channel_offset + out_channels) of dst [batch, dst_channels_total, OH, OW] in dst_layout
 *   (dst_elems = batch * dst_channels_total * OH * OW elements); exactly that window is written, nothing else, and the sources
 *   are only read inside their extents.  Limits, checked on the host before any GPU work, anything else returns 4 (unsupported):
 *   the three modes above, channels0 a multiple of 16 (>= 16), channels1 0 or a multiple of 16, out_channels a multiple of 32, an
 *   NHWC destination with dst_channels_total and dst_channel_offset in multiples of 4.  height, width >= 1; batch 0 .. 65535 (0:
 *   nothing to do).  Code 1: a null or misaligned pointer, bad sizes, packed_elems or dst_elems that do not fit the layer.
 *   The entry takes no extents of the sources, of scale and of shift and cannot tell a host pointer from a device pointer: the
 *   caller guarantees device buffers of batch * channels * height * width elements per source and out_channels floats each for
 *   scale and shift (the Python wrapper checks both and refuses host tensors). */
int bevamd_bev_conv_forward(const void* src0, int channels0, const void* src1, int channels1, int src_layout, int dtype, int batch,
                            int height, int width, int out_channels, int kernel, int stride, int mode, const void* packed,
                            long long packed_elems, const float* scale, const float* shift, void* dst, int dst_channels_total,
                            int dst_channel_offset, int dst_layout, long long dst_elems, void* stream);


/* The second half of a ResNet BasicBlock in eval mode (mmdet3d/models/backbones/resnet.py GeneralizedResNet over mmcv's BasicBlock):
 * conv2 3x3 + folded bn2 + residual + ReLU in ONE launch on 16-bit storage (dtype 0: fp16, 1: bf16) with fp32 accumulation on
 * v_mfma_f32_16x16x32; no workspace, no device synchronisation, no atomics, no split-K: equal calls give bit-equal results, a
 * sample's result does not depend on the batch, and the call can be captured in a graph.
 *
 * bevamd_res_block_forward: h [batch, channels, out_height, out_width] (the output of conv1 + bn1 + ReLU) in h_layout and x
 *   [batch, x_channels, x_height, x_width] (the block's input) in x_layout (0: NCHW, 1: NHWC = [batch, height, width, c]), both
 *   contiguous; an NHWC tensor is 16-byte aligned.  residual 0 (identity): x_channels = channels, x's map equals the output's and
 *   stride is 1; packed_d, scale_d and shift_d are not read (null, packed_d_elems 0).  residual 1 (downsample): a 1 x 1
 *   convolution of x with stride 1 or 2 and no padding, out_height = (x_height - 1) / stride + 1 and the width alike.
 *   packed2 holds exactly packed2_elems = channels * (channels / 32) * 9 * 32 16-bit elements and packed_d exactly packed_d_elems =
 *   channels * ceil(x_channels / 32) * 32, both 16-byte aligned, in the A-fragment order of bevamd_bev_conv_forward (mode 0,
 *   kernel 3 and kernel 1; zero where ci >= x_channels).  scale2, shift2, scale_d, shift_d: [channels] fp32, 16-byte aligned
 *   (scale = bn.weight / sqrt(running_var + eps), shift = bn.bias - running_mean * scale; never folded into the 16-bit weights).
 *     v = fma(sum_{chunk, tap, ci} w2 * h, scale2[co], shift2[co])                    h zero outside the map
 *     r = (float)x[b, co, p]                                                          (identity)
 *     r = fma(sum_{chunk, ci} wd * x[b, ci, stride * p], scale_d[co], shift_d[co])    (downsample)
 *     y[b, co, p] = round16(max(v + r, 0))
 *   in fp32 without contraction, ONE accumulator chain per sum in ascending (chunk, tap, ci).  dst [batch, channels, out_height,
 *   out_width] in dst_layout (dst_elems = batch * channels * out_height * out_width elements; an NHWC dst is 8-byte aligned):
 *   every element is written, nothing else, and h and x are only read inside their extents.  dst must not overlap h or x.
 *   Limits, checked on the host before any GPU work, anything else returns 4 (unsupported): residual 0 or 1, stride 1 or 2,
 *   channels a multiple of 32 (>= 32), x_channels a multiple of 16 (>= 16).  All maps >= 1 x 1; batch 0 .. 65535 (0: nothing to
 *   do, the tensors may be null).  Code 1: a null or misaligned pointer, a bad layout or dtype, bad sizes, maps that do not match
 *   the stride, an identity residual whose x differs from the output's shape, packed2_elems, packed_d_elems or dst_elems that do
 *   not fit the block, a dst that overlaps h or x.  The entry takes no extents of h, x, the scales and the shifts and cannot tell
 *   a host pointer from a device pointer: the caller guarantees device buffers of the sizes above (the Python wrapper checks
 *   them and refuses host tensors). */
int bevamd_res_block_forward(const void* h, int h_layout, const void* x, int x_layout, int x_channels, int x_height, int x_width,
                             int dtype, int batch, int channels, int out_height, int out_width, int residual, int stride,
                             const void* packed2, long long packed2_elems, const float* scale2, const float* shift2,
                             const void* packed_d, long long packed_d_elems, const float* scale_d, const float* shift_d, void* dst,
                             int dst_layout, long long dst_elems, void* stream);


/* The tail of a ResNet Bottleneck in eval mode (mmdet 2.x mmdet/models/backbones/resnet.py, the camera backbone `ResNet`): conv3
 * 1x1 + folded bn3 + residual + ReLU in ONE launch on 16-bit storage (dtype 0: fp16, 1: bf16) with fp32 accumulation on
 * v_mfma_f32_16x16x32; no workspace, no device synchronisation, no atomics, no split-K: equal calls give bit-equal results, a
 * sample's result does not depend on the batch, and the call can be captured in a graph.
 *
 * bevamd_bottleneck_tail_forward: h [batch, planes, out_height, out_width] (the output of conv2 + bn2 + ReLU) in h_layout and x
 *   [batch, x_channels, x_height, x_width] (the block's input) in x_layout (0: NCHW, 1: NHWC = [batch, height, width, c]), both
 *   contiguous; an NHWC tensor is 16-byte aligned.  residual 0 (identity): x_channels = channels, x's map equals the output's and
 *   stride is 1; packed_d, scale_d and shift_d are not read (null, packed_d_elems 0).  residual 1 (downsample): a 1 x 1
 *   convolution of x with stride 1 or 2 and no padding, out_height = (x_height - 1) / stride + 1 and the width alike.
 *   packed3 holds exactly packed3_elems = channels * ceil(planes / 32) * 32 16-bit elements and packed_d exactly packed_d_elems =
 *   channels * ceil(x_channels / 32) * 32, both 16-byte aligned, in the A-fragment order of bevamd_bev_conv_forward (mode 0,
 *   kernel 1; zero where ci >= planes or x_channels).  scale3, shift3, scale_d, shift_d: [channels] fp32, 16-byte aligned
 *   (scale = bn.weight / sqrt(running_var + eps), shift = bn.bias - running_mean * scale; never folded into the 16-bit weights).
 *     v = fma(sum_{chunk, ci} w3 * h[b, ci, p], scale3[co], shift3[co])
 *     r = (float)x[b, co, p]                                                          (identity)
 *     r = fma(sum_{chunk, ci} wd * x[b, ci, stride * p], scale_d[co], shift_d[co])    (downsample)
 *     y[b, co, p] = round16(max(v + r, 0))
 *   in fp32 without contraction, ONE accumulator chain per sum in ascending (chunk, ci).  dst [batch, channels, out_height,
 *   out_width] in dst_layout (dst_elems = batch * channels * out_height * out_width elements; an NHWC dst is 8-byte aligned):
 *   every element is written, nothing else, and h and x are only read inside their extents.  dst must not overlap h or x.
 *   channels need not equal 4 * planes.
 *   Limits, checked on the host before any GPU work, anything else returns 4 (unsupported): residual 0 or 1, stride 1 or 2,
 *   channels a multiple of 32 (>= 32), planes and x_channels multiples of 16 (>= 16).  All maps >= 1 x 1; batch 0 .. 65535 (0:
 *   nothing to do, the tensors may be null); batch * out_height * out_width below 2^31 - 128.  Code 1: a null or misaligned
 *   pointer, a bad layout or dtype, bad sizes, maps that do not match the stride, an identity residual whose x differs from the
 *   output's shape, packed3_elems, packed_d_elems or dst_elems that do not fit the block, a dst that overlaps h or x.  The entry
 *   takes no extents of h, x, the scales and the shifts and cannot tell a host pointer from a device pointer: the caller
 *   guarantees device buffers of the sizes above (the Python wrapper checks them and refuses host tensors). */
int bevamd_bottleneck_tail_forward(const void* h, int h_layout, int planes, const void* x, int x_layout, int x_channels, int x_height,
                                   int x_width, int dtype, int batch, int channels, int out_height, int out_width, int residual,
                                   int stride, const void* packed3, long long packed3_elems, const float* scale3, const float* shift3,
                                   const void* packed_d, long long packed_d_elems, const float* scale_d, const float* shift_d,
                                   void* dst, int dst_layout, long long dst_elems, void* stream);


/* The stem of a ResNet in eval mode (mmdet 2.x ResNet.forward: conv1, norm1, relu, maxpool): convolution 7 x 7 stride 2 padding 3
 * from 3 to 64 channels + folded BatchNorm + ReLU + max pooling 3 x 3 stride 2 padding 1 in ONE launch on 16-bit storage (dtype 0:
 * fp16, 1: bf16) with fp32 accumulation on v_mfma_f32_16x16x32; the convolution's map never reaches memory; no workspace, no
 * device synchronisation, no atomics: equal calls give bit-equal results, a sample's result does not depend on the batch, and the
 * call can be captured in a graph.
 *
 * bevamd_resnet_stem_forward: x [batch, 3, height, width] contiguous NCHW.  OH = (height - 1) / 2 + 1, PH = (OH - 1) / 2 + 1, the
 *   widths alike.  packed holds exactly packed_elems = 4 * 6 * 64 * 8 = 12288 16-bit elements, 16-byte aligned: element
 *   [mt][kstep][lane][j] is w[co = 16 mt + (lane & 15)][ci][ky][kx = j] with 7 ci + ky = 4 kstep + (lane >> 4), zero where kx = 7
 *   or 7 ci + ky >= 21.  scale, shift: [64] fp32, 16-byte aligned, as for bevamd_res_block_forward.
 *     c[b, co, cy, cx] = round16(max(fma(sum_k w * x[b, ci, 2 cy - 3 + ky, 2 cx - 3 + kx], scale[co], shift[co]), 0))
 *     y[b, co, ph, pw] = max over the cells (2 ph - 1 + dy, 2 pw - 1 + dx), dy, dx in 0 .. 2, inside the OH x OW map, of c
 *   x zero outside the image; fp32 without contraction, ONE accumulator chain per c in ascending k = 8 (7 ci + ky) + kx.  Rounding
 *   is monotone, so y equals the maximum of the fp32 values rounded once.  dst [batch, 64, PH, PW] in dst_layout (0: NCHW, 1:
 *   NHWC, then 16-byte aligned; dst_elems = batch * 64 * PH * PW): every element is written, nothing else, and x is only read
 *   inside its extent.  dst must not overlap x.
 *   Limits, checked on the host before any GPU work, anything else returns 4 (unsupported): in_channels 3, out_channels 64,
 *   kernel 7, stride 2, padding 3; pool_kernel 3, pool_stride 2, pool_padding 1, pool_ceil_mode 0.  Image >= 1 x 1; batch 0 ..
 *   65535 (0: nothing to do, x and dst may be null).  Code 1: a null or misaligned pointer, a bad layout or dtype, bad sizes,
 *   packed_elems or dst_elems that do not fit, a dst that overlaps x.  The entry takes no extents of x, scale and shift: the
 *   caller guarantees device buffers of the sizes above (the Python wrapper checks them and refuses host tensors). */
int bevamd_resnet_stem_forward(const void* x, int dtype, int batch, int in_channels, int height, int width, int out_channels,
                               int kernel, int stride, int padding, int pool_kernel, int pool_stride, int pool_padding,
                               int pool_ceil_mode, const void* packed, long long packed_elems, const float* scale,
                               const float* shift, void* dst, int dst_layout, long long dst_elems, void* stream);


/* The shifted-window attention of a Swin block in eval mode (mmdet 2.x mmdet/models/backbones/swin.py ShiftWindowMSA + WindowMSA
 * between the qkv and the proj Linear): pad, roll, window partition, q k^T, relative position bias, shift mask, softmax, attn v,
 * window reverse, roll back and crop in ONE launch on 16-bit storage (dtype 0: fp16, 1: bf16) with fp32 accumulation on
 * v_mfma_f32_16x16x32; no workspace, no device synchronisation, no atomics: equal calls give bit-equal results, a sample's result
 * does not depend on the batch, and the call can be captured in a graph.
 *
 * bevamd_window_attention_forward: qkv [batch, height, width, 3 * channels] contiguous, 16-byte aligned (qkv_elems elements), the
 *   qkv Linear of the un-padded, un-rolled token map with channel which * channels + head * 32 + d (which 0: q, 1: k, 2: v).
 *   pad_qkv [3 * channels] (pad_elems = 3 * channels), 16-byte aligned: the q, k, v of a padded token (the Linear's bias), or null
 *   with pad_elems 0 for zeros.  bias [heads, 49, 49] fp32 (bias_elems floats): the dense relative position bias [head][query][key].
 *   With Hp, Wp = height, width rounded up to 7, token (ty, tx) of window (wy, wx) is pixel y = (7 wy + ty + shift) mod Hp,
 *   x = (7 wx + tx + shift) mod Wp when y < height and x < width, else the padded token (which takes part as a key, and whose
 *   output is not written).  region(r) = 0 if r < Hp - 7, 1 if r < Hp - shift, else 2 of the rolled row r = 7 wy + ty, columns alike;
 *     logit[i][j] = fma(sum_d q_i[d] k_j[d], scale, bias[head][i][j]) + (shift > 0 and regions of i and j differ ? -100 : 0)
 *     p = exp(logit - max_j logit),  out_i[d] = round16((sum_j round16(p[i][j]) v_j[d]) / sum_j p[i][j])
 *   in fp32.  out [batch, height, width, channels] (out_elems elements), 8-byte aligned: every element is written, nothing else,
 *   and qkv is only read inside its extent.  out must not overlap qkv, pad_qkv or bias.
 *   Limits, checked on the host before any GPU work, anything else returns 4 (unsupported): window 7, head_dim 32.  channels =
 *   heads * 32, 0 <= shift < 7, map >= 1 x 1, batch >= 0 (0: nothing to do, qkv and out may be null).  Code 1: a null or misaligned
 *   pointer, a bad dtype, bad sizes, qkv_elems, pad_elems, bias_elems or out_elems that do not fit, an overlap.  The entry cannot
 *   tell a host pointer from a device pointer (the Python wrapper refuses host tensors). */
int bevamd_window_attention_forward(const void* qkv, long long qkv_elems, const void* pad_qkv, long long pad_elems, const float* bias,
                                    long long bias_elems, int dtype, int batch, int height, int width, int channels, int heads,
                                    int window, int head_dim, float scale, int shift, void* out, long long out_elems, void* stream);


/* The FFN half of a Swin block in eval mode (mmdet 2.x mmdet/models/backbones/swin.py SwinBlock.forward, `self.ffn(self.norm2(x),
 * identity=x)` over mmcv's FFN): LayerNorm, Linear C -> hidden, GELU (the erf form), Linear hidden -> C and the residual in ONE
 * launch on 16-bit storage (dtype 0: fp16, 1: bf16) with fp32 accumulation on v_mfma_f32_16x16x32; the hidden activations never
 * reach memory; no workspace, no device synchronisation, no atomics, no split-K: equal calls give bit-equal results, a token's
 * result does not depend on the tokens around it, and the call can be captured in a graph.
 *
 * bevamd_swin_ffn_forward: x [tokens, channels] contiguous, 16-byte aligned (x_elems elements).  gamma, beta [channels], b1
 *   [hidden], b2 [channels]: fp32, 16-byte aligned (the module's 16-bit parameters widened, which is exact).  Per row, in fp32
 *   without contraction, C = channels:
 *     mean = (sum_c x_c) / C     var = (sum_c (x_c - mean)^2) / C     rstd = 1 / sqrt(var + eps)        (two passes, c ascending)
 *     n_c  = round16(fma((x_c - mean) * rstd, gamma_c, beta_c))
 *     h_j  = round16(gelu(sum_c W1[j][c] n_c + b1_j))       gelu(t) = 0.5 t (1 + erf(t / sqrt 2))
 *     out_c = round16(x_c + (sum_j W2[c][j] h_j + b2_c))
 *   Each sum is ONE accumulator chain: the first in ascending k-steps of 32 channels, the second in ascending k-steps of 32 hidden
 *   units.  1 + erf is evaluated branch-free with an absolute error below 3e-7 (Abramowitz & Stegun 7.1.26 on the hardware
 *   reciprocal and exp2; csrc/ext/swin_ffn.hip), far below the rounding of h that follows.
 *   packed1, packed2: W1 [hidden, channels] and W2 [channels, hidden] in MFMA fragment order, 16-byte aligned, hidden * channels
 *   16-bit elements each (packed1_elems, packed2_elems).  With KS = channels / 32, CT = channels / 16, lane 0 .. 63, e 0 .. 7:
 *     packed1[((tile * KS + ks) * 64 + lane) * 8 + e] = W1[16 tile + (lane & 15)][32 ks + 8 (lane >> 4) + e]        tile < hidden / 16
 *     packed2[((s * CT + ct) * 64 + lane) * 8 + e]    = W2[16 ct + (lane & 15)][32 s + 16 (e >> 2) + 4 (lane >> 4) + (e & 3)]
 *                                                                                                  s < hidden / 32, ct < CT
 *   (the k order inside a step of packed2 is the order in which a lane holds the hidden units in the first product's result).
 *   out [tokens, channels] (out_elems elements), 16-byte aligned: every element is written, nothing else, and x is only read
 *   inside its extent.  out must not overlap x or any other operand.
 *   Limits, checked on the host before any GPU work, anything else returns 4 (unsupported) with the offending size in the error
 *   text: channels a multiple of 32 from 32 to 192, hidden a multiple of 32 from 32 to 768.  tokens 0 .. 2^34 (0: nothing to do, x
 *   and out may be null).  Code 1: a null or misaligned pointer, a bad dtype, an eps that is not finite and positive, element
 *   counts that do not fit, an overlap.  The entry cannot tell a host pointer from a device pointer (the Python wrapper refuses
 *   host tensors). */
int bevamd_swin_ffn_forward(const void* x, long long x_elems, const float* gamma, long long gamma_elems, const float* beta,
                            long long beta_elems, const void* packed1, long long packed1_elems, const float* b1, long long b1_elems,
                            const void* packed2, long long packed2_elems, const float* b2, long long b2_elems, int dtype,
                            long long tokens, int channels, int hidden, float eps, void* out, long long out_elems, void* stream);


/* One layer of the camera necks in eval mode (mmdet3d/models/necks/generalized_lss.py GeneralizedLSSFPN, models/necks/lss.py
 * LSSFPN): F.interpolate(bilinear, align_corners=True) + torch.cat + convolution + folded BatchNorm + optional ReLU in ONE launch
 * on 16-bit storage (dtype 0: fp16, 1: bf16) with fp32 accumulation on v_mfma_f32_16x16x32; no workspace, no device
 * synchronisation, no atomics, no split-K: equal calls give bit-equal results, a sample's result does not depend on the batch, and
 * the call can be captured in a graph.
 *
 * bevamd_neck_conv_forward: src0 [batch, channels0, height0, width0] and, when channels1 > 0, src1 [batch, channels1, height1,
 *   width1], each contiguous in its OWN layout (0: NCHW, 1: NHWC = [batch, h, w, c]; an NHWC source is 16-byte aligned) and with
 *   its OWN map.  The layer's input at the output resolution [out_height, out_width] is the channel concatenation of R(src0) then
 *   R(src1).  R is the identity (a copy, no arithmetic) for a source whose map equals the output map; otherwise the bilinear
 *   resampling with align_corners=True in exactly this fp32 arithmetic, no FMA contraction (h, w: the source's map, H, W: the
 *   output's, (Y, X) the output pixel):
 *     ry = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0                                              (rx likewise)
 *     sy = ry * (float)Y;  y0 = min((int)sy, h - 1);  y1 = y0 + (y0 < h - 1);  ly = sy - (float)y0;  hy = 1.f - ly   (x likewise)
 *     v  = hy * (hx * a[y0][x0] + lx * a[y0][x1]) + ly * (hx * a[y1][x0] + lx * a[y1][x1])
 *   v is rounded ONCE to the storage type and that 16-bit value is the MFMA operand; any ratio is served, downsampling included.
 *   kernel 1 or 3, stride 1, padding kernel / 2: the zero padding applies AFTER the resampling (positions outside the output map
 *   are zero).  With Cin = channels0 + channels1 and nch = ceil(Cin / 32), packed holds exactly packed_elems = out_channels * nch *
 *   kernel^2 * 32 16-bit elements, 16-byte aligned, in the A-fragment order of bevamd_bev_conv_forward (mode 0).  scale, shift:
 *   [out_channels] fp32, 16-byte aligned, never folded into the 16-bit weights.
 *     y[b, co, p] = round16(relu ? max(fma(acc, scale[co], shift[co]), 0) : fma(acc, scale[co], shift[co]))
 *   with ONE fp32 accumulator chain per element in ascending (chunk, tap, ci).  y is written into the channels
 *   [dst_channel_offset, dst_channel_offset + out_channels) of dst [batch, dst_channels_total, out_height, out_width] in dst_layout
 *   (dst_elems = batch * dst_channels_total * out_height * out_width elements; an NHWC dst is 8-byte aligned); exactly that window
 *   is written, nothing else, and the sources are only read inside their extents.  Limits, checked on the host before any GPU
 *   work, anything else returns 4 (unsupported): kernel 1 or 3, channels0 a multiple of 16 (>= 16), channels1 0 or a multiple of
 *   16, out_channels a multiple of 32, an NHWC destination with dst_channels_total and dst_channel_offset in multiples of 4.  All
 *   maps >= 1 x 1 and at most 2^31 - 1 pixels; batch 0 .. 65535 (0: nothing to do).  Code 1: a null or misaligned pointer, a bad
 *   layout or dtype, bad sizes, packed_elems or dst_elems that do not fit the layer.  The entry takes no extents of the sources,
 *   of scale and of shift and cannot tell a host pointer from a device pointer: the caller guarantees device buffers of batch *
 *   channels * height * width elements per source and out_channels floats each for scale and shift (the Python wrapper checks
 *   both and refuses host tensors). */
int bevamd_neck_conv_forward(const void* src0, int channels0, int height0, int width0, int layout0, const void* src1, int channels1,
                             int height1, int width1, int layout1, int dtype, int batch, int out_height, int out_width,
                             int out_channels, int kernel, const void* packed, long long packed_elems, const float* scale,
                             const float* shift, int relu, void* dst, int dst_channels_total, int dst_channel_offset, int dst_layout,
                             long long dst_elems, void* stream);


/* The learned nets of the camera -> BEV view transform in eval mode (mmdet3d/models/vtransforms/depth_lss.py:43-97, lss.py:63-75)
 * on 16-bit operands (dtype 0: fp16, 1: bf16) with fp32 accumulation on v_mfma_f32_16x16x32.  No device synchronisation, no
 * allocation, no atomics, no split-K: equal calls give bit-equal results, a sample's result does not depend on the batch, and both
 * calls can be captured in a graph.  Limits are checked on the host before any GPU work; batch 0 .. 65535 (0: nothing to do).
 *
 * bevamd_cam_depth_stem_forward (2 launches): DepthLSSTransform.dtransform, Conv2d(1, 8, 1), Conv2d(8, 32, 5, stride 4, padding 2),
 *   Conv2d(32, 64, 5, stride 2, padding 2), each with bias, eval-mode BatchNorm2d and ReLU.  depth [batch, height, width] fp32
 *   (depth_elems elements), read in place; out [batch, OH3, OW3, 64] NHWC 16-bit with OH2 = (height - 1) / 4 + 1, OH3 = (OH2 - 1) / 2
 *   + 1 and the widths alike; scratch [batch, OH2, OW2, 32] 16-bit holds the layer-2 map (written in full, then read).  Both are
 *   16-byte aligned and of exactly scratch_elems / out_elems elements.
 *     a1[c]  = round16(max(fma(d, scale1[c], shift1[c]), 0))                         (never stored; fp32, one rounding)
 *     a2[co] = round16(max(fma(sum_{tap, ci} w2 * a1, scale2[co], shift2[co]), 0))   a1 taken as ZERO outside the image
 *     y[co]  = round16(max(fma(sum_{tap, ci} w3 * a2, scale3[co], shift3[co]), 0))   a2 taken as zero outside its map
 *   scale_i = bn.weight / sqrt(running_var + eps), shift_i = bn.bias + (conv.bias - running_mean) * scale_i, fp32 arrays of 8, 32
 *   and 64 floats (those of layers 2 and 3 16-byte aligned), never folded into the 16-bit weights.  packed2: exactly 32 * 224
 *   elements, the A-fragment order of bevamd_bev_conv_forward for a 1 x 1 layer of 200 input channels k = 8 tap + ci (tap = 5 ky +
 *   kx), zero for k >= 200; packed3: exactly 64 * 800 elements, the same order for the 5 x 5 layer of 32 channels.  Any height,
 *   width >= 1.  Code 1: a null or misaligned pointer, a dtype other than 0 / 1, element counts that do not fit the sizes.
 * bevamd_cam_depth_head_forward (1 launch): Conv2d(in_channels, depth_bins + context_channels, 1) with bias, softmax over the first
 *   depth_bins rows, the split.  x [batch, height, width, in_channels] NHWC 16-bit, 16-byte aligned; packed: (depth_bins +
 *   context_channels, rounded up to a multiple of 16) * in_channels elements in the same A-fragment order (1 x 1), zero rows past
 *   the last; bias [depth_bins + context_channels] fp32.  depth [batch, depth_bins, height, width] fp32, context [batch, height,
 *   width, context_channels] fp32, every element written, nothing else.  z = acc + bias in fp32, never stored;
 *   depth = exp(z - max z) / sum exp(z - max z) over exactly the depth rows (expf within 1 ulp, IEEE division, the sum over a lane's
 *   rows in ascending order, then over the four lane groups); context = z.  Served, anything else returns 4 (unsupported):
 *   in_channels a multiple of 32 up to 512, depth_bins 1 .. 128, context_channels a multiple of 4 up to 128; any height, width >= 1.
 *   Code 1 as above. */
int bevamd_cam_depth_stem_forward(const float* depth, long long depth_elems, int batch, int height, int width, int dtype,
                                  const float* scale1, const float* shift1, const void* packed2, long long packed2_elems,
                                  const float* scale2, const float* shift2, const void* packed3, long long packed3_elems,
                                  const float* scale3, const float* shift3, void* scratch, long long scratch_elems, void* out,
                                  long long out_elems, void* stream);
int bevamd_cam_depth_head_forward(const void* x, long long x_elems, int batch, int height, int width, int in_channels, int depth_bins,
                                  int context_channels, int dtype, const void* packed, long long packed_elems, const float* bias,
                                  float* depth, long long depth_elems, float* context, long long context_elems, void* stream);


/* The non-learned end of CenterHead (mmdet3d/models/heads/bbox/centerpoint.py:637-884 get_bboxes / get_task_detections and
 * CenterPointBBoxCoder.decode, core/bbox/coders/centerpoint_bbox_coders.py:62-225).  Nothing below synchronises the device or
 * reads anything back; every call is a fixed number of launches on `stream` for ANY number of tasks and samples and can be
 * captured in a graph.  Tasks travel as HOST tables (at most 16 tasks of at most 8 classes); the segment of every per-row array
 * is (sample, task): row = (sample * num_tasks + task) * max_num + k.
 *
 * bevamd_centerpoint_select: heatmaps: HOST array of num_tasks DEVICE pointers [batch, task_classes[t], height, width] fp32,
 *   FINITE; apply_sigmoid 1: logits (get_bboxes), 0: scores (the coder's decode).  Per segment the max_num (1 .. 1024, at most
 *   height * width, where the reference's per-class topk raises) largest scores in STABLE descending order: equal scores in
 *   ascending flat index c * height * width + cell, which is what the reference's two-level top-K yields wherever its answer is
 *   defined.  top_flat [batch, num_tasks, max_num] int32 (that flat index), top_score fp32.  Two launches.
 *   ws: bevamd_centerpoint_select_workspace_bytes(batch, sum of task_classes, height, width); it needs no initialisation.
 * bevamd_centerpoint_decode: one launch, one thread per row.  maps: HOST array of 5 * num_tasks DEVICE pointers, per task
 *   {reg [batch, 2, H, W] or NULL, height [batch, 1, H, W], dim [batch, 3, H, W], rot [batch, 2, H, W], vel [batch, 2, H, W] or
 *   NULL} (reg / vel: for every task or for none), read at the selected cell only.  boxes [rows, 7 or 9 with vel] =
 *   ((cell / W + reg0) * osf * vs0 + pc0, (cell % W + reg1) * osf * vs1 + pc1 (+ 0.5 each without reg; the FIRST coordinate is
 *   the row, as in the reference), height (- dim2 * 0.5 with bottom_centre, centerpoint.py:746), dim (exp(dim) with norm_bbox), atan2(rot0, rot1), vel) in the reference's
 *   fp32 operation order without FMA contraction; exp / atan2 are rounded once from double.  labels int32: class within the task
 *   + the classes of the tasks before it.  live uint8 = inside post_center_range (HOST 6 floats, inclusive, on x, y and the
 *   UNSHIFTED height) AND (use_coder_threshold == 0 OR score > coder_threshold) AND, for a task with task_rotate[t] != 0,
 *   (use_head_threshold == 0 OR score >= head_threshold).  post_ok uint8 = 1, or for a task_rotate task inside
 *   post_center_limit_range (HOST 6 floats or NULL: no test).  coder: HOST {out_size_factor, voxel_size[0], voxel_size[1],
 *   pc_range[0], pc_range[1]} as fp32.  A top_flat outside the task's map yields a dead row of zeros.
 * bevamd_rotate_nms_segments: nms_gpu (ops/iou3d/iou3d_utils.py:23-48 over iou3d_kernel.cu:264-345 and iou3d.cpp:96-133) on
 *   num_segments segments of rows_per_segment (1 .. 1024; more: 4, unsupported) rows ALREADY in descending score, one workgroup
 *   each; segment s belongs to task s % num_tasks.  boxes [rows, box_width >= 7] (x, y, z, w, l, h, yaw, ...): the BEV box is the
 *   LiDAR convention's (x - w / 2, y - l / 2, x + w / 2, y + l / 2, yaw) with w and l multiplied by
 *   task_scale[task * 8 + labels[row] - task_label_base[task]] (HOST tables; task_scale NULL: 1, labels may then be NULL).  The
 *   live rows (live NULL: all) are cut to the first pre_max_size; greedy: a row is dropped when an earlier kept row has rotated
 *   IoU > task_thresh[task], in the arithmetic of bevamd_iou3d_nms; the first post_max_size kept rows stay, then those with
 *   post_ok == 0 (NULL: none) are dropped.  A task with task_enabled[t] == 0 (NULL: all enabled) keeps nothing.  keep [rows]
 *   uint8, seg_counts [num_segments] int32.  No workspace, no K x K mask. */
size_t bevamd_centerpoint_select_workspace_bytes(int batch, int total_classes, int height, int width);
int bevamd_centerpoint_select(const void* const* heatmaps, const int* task_classes, int num_tasks, int batch, int height,
                              int width, int max_num, int apply_sigmoid, int* top_flat, float* top_score, void* ws,
                              size_t ws_bytes, void* stream);
int bevamd_centerpoint_decode(const void* const* maps, const int* task_classes, const int* task_rotate, int num_tasks, int batch,
                              int height, int width, int max_num, const int* top_flat, const float* top_score, int norm_bbox,
                              int bottom_centre, const float* coder, const float* post_center_range, float coder_threshold,
                              int use_coder_threshold, float head_threshold, int use_head_threshold,
                              const float* post_center_limit_range, float* boxes, int* labels, unsigned char* live,
                              unsigned char* post_ok, void* stream);
int bevamd_rotate_nms_segments(const float* boxes, int box_width, const int* labels, const unsigned char* live,
                               const unsigned char* post_ok, int num_segments, int rows_per_segment, int num_tasks,
                               const int* task_enabled, const float* task_thresh, const int* task_label_base,
                               const float* task_scale, int pre_max_size, int post_max_size, unsigned char* keep,
                               int* seg_counts, void* stream);


/* Training targets of the two heads: CenterHead.get_targets_single (mmdet3d/models/heads/bbox/centerpoint.py:432-582) and the
 * dense heatmap of TransFusionHead.get_targets_single (transfusion.py:526-573), over core/utils/gaussian.py.  Nothing below
 * synchronises the device or reads anything back.  LAUNCHES: bevamd_centerhead_targets 3 (zero, slots, draw),
 * bevamd_heatmap_targets 2 (zero, draw), on `stream`, for ANY batch, num_rows and box contents; both can be captured in a graph.
 * No workspace.  The heatmap is zeroed inside the call and every other output element is written on every call.
 *
 * Packed inputs: boxes [num_rows, box_dim] fp32 in the LiDAR layout (bottom centre x, y, z; dx, dy, dz; yaw; vx, vy when box_dim
 *   is 9; 7: the velocity columns of anno_box are 0), labels [num_rows] int64, offsets [batch + 1] int32 ON THE DEVICE: sample b
 *   owns the rows [offsets[b], offsets[b + 1]).  max_boxes_per_sample: the caller's HOST bound, 1 .. 1024 (more: 4, unsupported,
 *   before any GPU work).  A sample with more rows than the bound (or whose offsets do not name a range of the arrays) produces
 *   all-zero outputs and overflow[b] = 1; every other entry of overflow [batch] int32 is 0.
 * pc_range, voxel_size: HOST, 2 floats each (the fp32 values of torch.tensor(train_cfg[...])); map_size: the feature map is
 *   map_size x map_size (grid_size // out_size_factor; SQUARE only: the reference draws on a [size[1], size[0]] plane at
 *   (row cell_x, column cell_y) and indexes it with cell_x * size[1] + cell_y, which agree only on square maps).
 * Shared semantics, in the reference's fp32 operation order without FMA contraction and with correctly rounded divide / sqrt:
 *   width = dx / voxel_size[0] / out_size_factor, length = dy / voxel_size[1] / out_size_factor; a box is skipped unless both are
 *   > 0; radius = max(min_radius, int(gaussian_radius((length, width), gaussian_overlap))) as CPU fp32 torch evaluates it, the
 *   Python-float constants formed in double and rounded to fp32; coor = (x - pc_range) / voxel_size / out_size_factor, the cell is
 *   coor truncated toward zero (a coordinate in (-1, 0) lands in cell 0); a cell outside the map skips the box.  The Gaussian
 *   exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2 radius + 1) / 6, is evaluated in double, cut below eps, rounded once to fp32 and
 *   combined by maximum over the window clipped to the map, at row cell_x, column cell_y of the box's plane.
 * bevamd_centerhead_targets: task t owns the labels [flag_t, flag_t + task_classes[t]) (HOST table, at most 16 tasks, 64 classes
 *   in all); other labels, -1 included, are ignored.  Slot k of (task, sample) is the k-th box of the task in CLASS-MAJOR order,
 *   stable within a class; only the first max_objs (the caller's max_objs * dense_reg) are processed; a skipped box leaves its
 *   slot zero with mask 0.  heatmap: per task a contiguous [batch, task_classes[t], size, size] block, tasks in order;
 *   anno_box [num_tasks, batch, max_objs, 10] = (coor_x - cell_x, coor_y - cell_y, z + dz * 0.5, dims (log with norm_bbox),
 *   sin(yaw), cos(yaw), vx, vy), log / sin / cos rounded once from double; ind [num_tasks, batch, max_objs] int64 =
 *   cell_x * size + cell_y; mask uint8.
 * bevamd_heatmap_targets: heatmap [batch, num_classes, size, size], plane = label.  Where the reference is undefined (a centre
 *   cell outside the map or a label outside [0, num_classes): its slices turn negative and index from the end) the box is SKIPPED. */
int bevamd_centerhead_targets(const float* boxes, const long long* labels, const int* offsets, int num_rows, int box_dim,
                              int batch, int max_boxes_per_sample, const int* task_classes, int num_tasks, int max_objs,
                              const float* pc_range, const float* voxel_size, int out_size_factor, int map_size,
                              double gaussian_overlap, int min_radius, int norm_bbox, float* heatmap, float* anno_box,
                              long long* ind, unsigned char* mask, int* overflow, void* stream);
int bevamd_heatmap_targets(const float* boxes, const long long* labels, const int* offsets, int num_rows, int box_dim, int batch,
                           int max_boxes_per_sample, int num_classes, const float* pc_range, const float* voxel_size,
                           int out_size_factor, int map_size, double gaussian_overlap, int min_radius, float* heatmap,
                           int* overflow, void* stream);


/* The assignment end of TransFusionHead.get_targets (mmdet3d/models/heads/bbox/transfusion.py:357-524, 575 over
 * core/bbox/assigners/hungarian_assigner.py:13-35, 82-142, BaseInstance3DBoxes.overlaps of core/bbox/structures/base_box3d.py:378-445
 * and mmdet 2.x's FocalLossCost / ClassificationCost): match costs, a batched rectangular linear sum assignment, and the target
 * rows that follow from it.  Nothing below synchronises the device, reads anything back or takes a workspace; every output
 * element is written on every call; all of it can be captured in one graph.  LAUNCHES: bevamd_match_costs 2 (sizes, costs),
 * bevamd_linear_sum_assignment 1, bevamd_transfusion_assign_targets 1.  Problem n = sample * layers + layer.
 * Ground truth is packed as for the head targets above (boxes [num_rows, 7|9] fp32 LiDAR layout, labels [num_rows] int64,
 * offsets [batch + 1] int32 ON THE DEVICE, the HOST bound max_boxes_per_sample 1 .. 1024; more: 4, unsupported, before any launch).
 * STATUS bits (per problem): 1 a live cost entry is not finite; 2 a ground-truth label outside [0, classes); 4 the sample has more
 *   boxes than the bound or its offsets name no range of the arrays (its live count is 0); 8 the solver's loop bound was reached or
 *   a live size lies outside the buffer.
 *
 * bevamd_match_costs: boxes [batch, layers * num_proposals, box_dim] fp32 DECODED boxes (bevamd_transfusion_decode with
 *   num_proposals = layers * K; NULL when neither box cost is asked for), logits [batch, classes, layers * num_proposals] fp32
 *   (NULL with cls_mode 0).  cost, iou [batch, layers, num_proposals, max_boxes_per_sample] fp32: slot g of problem n is ground
 *   truth offsets[sample] + g; slots past the live count are 0.  num_gt [batch * layers] int32: the live count (the `cols` of the
 *   solver); status [batch * layers] int32.  cost = cls + reg + iou_cost, each term in the reference's fp32 operation order without
 *   FMA contraction, sigmoid / log / pow / exp evaluated in double and rounded once:
 *     cls_mode 1 FocalLossCost: p = sigmoid(logit[label]); neg = -log(1 - p + eps) * (1 - alpha) * p^gamma;
 *       pos = -log(p + eps) * alpha * (1 - p)^gamma; (pos - neg) * cls_weight.  cls_mode 2 ClassificationCost:
 *       -softmax(logits over classes)[label] * cls_weight.  A label outside [0, classes) makes the entry NaN and sets bits 1 and 2.
 *     use_reg BBoxBEVL1Cost: (|dx| + |dy|) * reg_weight of (xy - pc_range[0:2]) / (pc_range[3:5] - pc_range[0:2]); pc_range: HOST,
 *       6 floats (the fp32 values of the tensor the reference builds).
 *     use_iou IoU3DCost: -iou * iou_weight; iou: BEV overlap of (x - dx / 2, y - dy / 2, x + dx / 2, y + dy / 2, yaw) in the
 *       arithmetic of bevamd_iou3d_boxes_overlap_bev, times clamp(min(z + dz) - max(z), 0), over
 *       clamp(v1 + v2 - overlap, 1e-8) with v = dx * dy * dz.  Without use_iou `iou` is 0.
 * bevamd_linear_sum_assignment: scipy.optimize.linear_sum_assignment for num_problems problems over cost
 *   [num_problems, max_rows, max_cols] fp32 with the live sizes rows / cols [num_problems] int32 READ FROM DEVICE MEMORY (NULL: the
 *   full side), so that a graph replay may change them; entries outside the live block are never read.  max_rows, max_cols
 *   1 .. 1024 (more: 4, unsupported, before any launch).  col4row [num_problems, max_rows] int32: the column of every live row, -1
 *   for an unmatched row and for rows past the live count; min(rows, cols) rows are matched.  Shortest augmenting paths with dual
 *   variables (Jonker-Volgenant / Crouse), over the smaller side, duals and path costs in fp64: optimal for the given fp32 matrix;
 *   among equal path costs an unmatched column is preferred, then the lower one, so equal-cost optima may differ from scipy's.
 *   One wave per problem; the cost block is staged in LDS when max_rows x max_cols x 4 bytes fit beside the state (12 x the
 *   smaller + 28 x the larger side, in bytes) in 64 KiB, otherwise read through L2.  Every loop is bounded (an augmentation visits at most `cols` columns, there are
 *   `rows` augmentations): a problem with a non-finite live entry (status 1), with a live size outside the buffer or over the loop
 *   bound (status 8) returns all rows -1; other problems of the batch are not affected.  status [num_problems] int32.
 * bevamd_transfusion_assign_targets: rows p = layer * num_proposals + k of every sample from col4row [batch * layers,
 *   num_proposals] and iou (as above): labels [batch, P] int64 (num_classes, or the matched label), label_weights [batch, P] int64
 *   (1, or pos_weight > 0 on positives), bbox_targets [batch, P, code_size] fp32 = TransFusionBBoxCoder.encode of the matched box
 *   ((x - coder[0]) / coder[2], (y - coder[1]) / coder[3], z + dz * 0.5, log dims, sin, cos yaw (rounded once from double), vx, vy
 *   with code_size 10, which needs 9 box columns; coder: HOST, 4 doubles {pc_range[0], pc_range[1], out_size_factor *
 *   voxel_size[0], out_size_factor * voxel_size[1]}, each rounded to fp32 as the reference's scalar operands are), bbox_weights
 *   (1 on positive rows), ious [batch, P] (the matched pair's iou clamped to [0, 1]), all zero on negative rows.  flags [batch]
 *   int32: the OR of the sample's status words (status_cost may be NULL) and bit 4; a flagged sample is all negative (so is one
 *   without ground truth, where the reference raises).  num_pos: one int32; matched_ious: one fp32, the mean over samples of
 *   sum(ious[pos]) / max(n_pos, 1), summed in a fixed order. */
int bevamd_match_costs(const float* boxes, const float* logits, const float* gt_boxes, const long long* gt_labels,
                       const int* offsets, int num_rows, int box_dim, int batch, int layers, int num_proposals, int classes,
                       int max_boxes_per_sample, int cls_mode, float cls_weight, double alpha, double gamma, float eps,
                       int use_reg, float reg_weight, int use_iou, float iou_weight, const float* pc_range, float* cost,
                       float* iou, int* num_gt, int* status, void* stream);
int bevamd_linear_sum_assignment(const float* cost, const int* rows, const int* cols, int num_problems, int max_rows,
                                 int max_cols, int* col4row, int* status, void* stream);
int bevamd_transfusion_assign_targets(const int* col4row, const float* iou, const int* status_cost, const int* status_lsa,
                                      const float* gt_boxes, const long long* gt_labels, const int* offsets, int num_rows,
                                      int box_dim, int batch, int layers, int num_proposals, int max_boxes_per_sample,
                                      int num_classes, int code_size, long long pos_weight, const double* coder,
                                      long long* labels, long long* label_weights, float* bbox_targets, float* bbox_weights,
                                      float* ious, int* flags, int* num_pos, float* matched_ious, void* stream);


/* Map segmentation metrics.  Replace the counting of NuScenesDataset.evaluate_map (mmdet3d/datasets/nuscenes_dataset.py:498-530).
 * bevamd_seg_iou_counts (2 launches: zero, count): pred [samples, classes, hw] fp32; label of the same shape, label_dtype 0 fp32
 *   / 3 uint8 or bool, non-zero is true (as with .bool()); thresholds: DEVICE fp32 [num_thresholds], 1 .. 16.  counts [classes,
 *   num_thresholds, 3] int64 = tp, fp, fn over samples and cells, the prediction being `pred >= threshold` in fp32 (a NaN is below
 *   every threshold).  The call zeroes counts itself.  64-bit integer atomics: exact and independent of arrival order.  classes
 *   1 .. 1024, samples * hw <= 2^36; code 1 for bad sizes, more than 16 thresholds or a null pointer, code 4 for another
 *   label_dtype, both before any GPU work.  No synchronisation, no read-back, no workspace. */
int bevamd_seg_iou_counts(const float* pred, const void* label, int label_dtype, int samples, int classes, long long hw,
                          const float* thresholds, int num_thresholds, long long* counts, void* stream);

/* Fused multi-head attention of the TransFusion decoder layer (mmdet3d/models/utils/transformer.py:244-493), head dimension 16:
 * out = dropout(softmax(q k^T / 4)) v per head, the logits never stored.  q [B, L, H * 16], k, v [B, S, H * 16] contiguous and
 * 16-byte aligned; out [B, L, H * 16] in the input dtype (0 fp32, 1 fp16); lse [B, H, L] fp32 = log sum exp of the scaled logits.
 * The softmax and both accumulations are fp32 (v_mfma_f32_16x16x4_f32).  Shapes: 1 <= B <= 4095, 1 <= H <= 16, 1 <= L <= 1024,
 * 1 <= S <= 2^20; anything else is code 1 before any GPU work (code 4 for another dtype, code 2 for a short workspace).
 * bevamd_mha_workspace_bytes: host only; what forward and backward need (the larger); 0 for a shape the entry points reject.
 * bevamd_mha_plan: host only; plan4 = {forward splits, keys per split (a multiple of 64), backward key blocks, keys per block (a
 *   multiple of 256)}: functions of (B, H, L, S) alone, so equal calls are bit-equal and a captured graph replays.
 * bevamd_mha_forward (2 launches): every split keeps a running (max, sum, out) per query; the second launch merges the splits in
 *   order.  dropout_p in [0, 1): weight (b * H + h, query, key) is kept when a counter hash of (seed, b * H + h, query, key) reaches
 *   dropout_p * 2^32, kept weights are scaled by 1 / (1 - p), the row sum uses the undropped weights.
 *   stats (may be NULL): [2, B, H, L] fp32 = lse in two terms, the row maximum and the log of the row sum, which the backward reads
 *   (their fp32 sum, lse, loses digits to a large maximum).
 * bevamd_mha_backward (3 launches; fp32): delta = rowsum(dout * out); the weights are recomputed from stats, dS = P (dP - delta), with
 *   the forward's mask from the same seed.  A workgroup owns a block of keys: dk, dv are written once; dq goes to one partial buffer
 *   per key block that the last launch sums in block order.  No floating-point atomics.
 * Both are asynchronous on `stream`: no synchronisation, no allocation, no read-back. */
size_t bevamd_mha_workspace_bytes(int B, int H, int L, int S);
int bevamd_mha_plan(int B, int H, int L, int S, int* plan4);
int bevamd_mha_forward(const void* q, const void* k, const void* v, int B, int H, int L, int S, int dtype, double dropout_p,
                       unsigned long long seed, void* out, float* lse, float* stats, void* workspace, size_t workspace_bytes,
                       void* stream);
int bevamd_mha_backward(const float* q, const float* k, const float* v, const float* out, const float* stats, const float* dout, int B,
                        int H, int L, int S, double dropout_p, unsigned long long seed, float* dq, float* dk, float* dv,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Losses of the detection heads (csrc/ext/head_losses.hip).  Replace TransFusionHead.loss (mmdet3d/models/heads/bbox/
 * transfusion.py:612-711), CenterHead.loss (centerpoint.py:597-633) and the mmdet 2.x losses they call: gaussian_focal_loss,
 * py_sigmoid_focal_loss and l1_loss under weight_reduce_loss(reduction="mean", avg_factor).  All tensors fp32 and contiguous unless
 * said otherwise.  Every cell term is evaluated in double from the fp32 inputs, summed in fp64 per workgroup and combined in a fixed
 * order; the result is loss_weight * (fp32(sum) / avg) in fp32.  No floating-point atomics; every output element is written on
 * every call; asynchronous on `stream`: no synchronisation, no allocation, no read-back, so all of it can be captured in a graph.
 * Code 1 (bad sizes, a null pointer, more than 16 maps / tasks, a code of other than 8 / 10 columns) and code 4 (another dtype
 * code, max_objs over 1024) are returned with an error string before any GPU work.
 *
 * bevamd_head_loss_plan: host only.  plan2 = {workgroups, cells per workgroup pass} for a map of `cells` cells (1 .. 2^40): the
 *   workgroups are min(ceil(cells / pass), 1024); workgroup w owns the passes w, w + workgroups, ... of the map.
 * bevamd_gaussian_focal_forward (2 launches: partials, finish): pred, target, cells: HOST arrays of num_maps (1 .. 16) device
 *   pointers / cell counts; the bases need 4-byte alignment only (16-byte accesses of pred, and of grad where it shares pred's
 *   alignment, run between a scalar head and tail; target is read wide where it is aligned at the same cells).  Per cell, p = clamp(sigmoid(x), 1e-4, 1 - 1e-4) with pred_is_logit 1 (clip_sigmoid), p =
 *   x with 0; loss = -log(p + 1e-12) (1 - p)^alpha [t == 1] - log(1 - p + 1e-12) p^alpha (1 - t)^gamma.  num_pos [num_maps] fp32 =
 *   the count of t == 1; loss [num_maps] = loss_weight * (sum / avg) with avg = *avg[t] when the HOST array avg and its entry t are
 *   not NULL (a device scalar), else max(num_pos[t], 1).  partials: num_maps x W x 2 doubles, W = the plan's workgroups for the
 *   LARGEST map of the call; every entry that is read is written first.
 * bevamd_gaussian_focal_backward (1 launch): grad[t] (HOST array of device pointers, as pred) = d loss[t] / d pred[t] *
 *   grad_out[t], in full: the per-cell derivative is recomputed from pred and target, is 0 where the clamp is active, is rounded once
 *   to fp32 and multiplied by the fp32 grad_out[t] * loss_weight / avg; num_pos: the forward's output.
 * bevamd_transfusion_layer_losses_forward (1 launch) / _backward (1 launch): the per-decoder-layer losses over P = L * K proposals,
 *   layer l owning the proposals [l K, (l + 1) K).  Either half may be left out (scores NULL / center NULL), not both.
 *   Class: scores [B, C, P] read in place; labels [B, P] int64, C = background (an all-zero one-hot row), a value outside [0, C] makes
 *   the layer's loss and the row's gradients NaN; label_weights [B, P] fp32 (weight_dtype 0) or int64 (2).  loss_cls [L] = cls_weight
 *   * sum(BCE_with_logits(x, y) (alpha y + (1 - alpha)(1 - y)) pt^gamma w) / avg, pt = (1 - s) y + s (1 - y), s = sigmoid(x).
 *   Boxes: center [B, 2, P], height [B, 1, P], dim [B, 3, P], rot [B, 2, P], vel [B, 2, P] (NULL with D = 8, required with D = 10)
 *   read in place as the columns 0-1, 2, 3-5, 6-7, 8-9 of the code; with height, dim, rot and vel all NULL `center` is instead one
 *   packed [B, P, D] tensor, D 1 .. 16.  bbox_targets, bbox_weights [B, P, D]; code_weights: HOST, D floats (NULL: ones).  loss_box
 *   [L] = box_weight * sum(|pred - target| fp32(bbox_weights * code_weights)) / avg.
 *   avg = *avg_cls / *avg_box (device fp32 scalars) where given, else max(*num_pos, 1) with num_pos a device int32.
 *   Backward: grad_cls, grad_box [L] device; grad_scores [B, C, P] and one gradient per piece (packed: grad_center alone), in full.
 * bevamd_centerhead_box_loss_forward (1 launch) / _backward (2 launches: zero, scatter): maps: HOST array of 5 * num_tasks device
 *   pointers, task-major {reg [B, 2, hw], height [B, 1, hw], dim [B, 3, hw], rot [B, 2, hw], vel [B, 2, hw]}, read only at the cells
 *   ind[t] [B, max_objs] int64 (an index outside [0, hw) makes the task's loss NaN and gets no gradient); target[t] [B, max_objs,
 *   10]; mask[t] [B, max_objs] uint8; num_tasks 1 .. 16, max_objs 1 .. 1024; code_weights: HOST, 10 floats.  weight = mask * (target
 *   is not NaN) * code_weights; avg [num_tasks] = fp32(mask.sum()) + 1e-4 (an output, which the backward reads); loss [num_tasks] =
 *   loss_weight * sum(|pred - target| weight) / avg.  A NaN target gives a NaN loss, as the reference's |pred - NaN| * 0 does.
 *   Backward: the 5 * num_tasks gradient maps (grad_maps, laid out as maps) are zeroed inside the call; slots of a sample that share
 *   a cell are summed in fp32 in slot order and written once by the first of them. */
int bevamd_head_loss_plan(long long cells, int* plan2);
int bevamd_gaussian_focal_forward(const float* const* pred, const float* const* target, const long long* cells, int num_maps,
                                  int pred_is_logit, double alpha, double gamma, float loss_weight, const float* const* avg,
                                  double* partials, float* loss, float* num_pos, void* stream);
int bevamd_gaussian_focal_backward(const float* const* pred, const float* const* target, const long long* cells, int num_maps,
                                   int pred_is_logit, double alpha, double gamma, float loss_weight, const float* const* avg,
                                   const float* num_pos, const float* grad_out, float* const* grad, void* stream);
int bevamd_transfusion_layer_losses_forward(const float* scores, const long long* labels, const void* label_weights, int weight_dtype,
                                            const float* center, const float* height, const float* dim, const float* rot,
                                            const float* vel, const float* bbox_targets, const float* bbox_weights,
                                            const float* code_weights, const int* num_pos, const float* avg_cls, const float* avg_box,
                                            int B, int C, int L, int K, int D, double alpha, double gamma, float cls_weight,
                                            float box_weight, float* loss_cls, float* loss_box, void* stream);
int bevamd_transfusion_layer_losses_backward(const float* scores, const long long* labels, const void* label_weights, int weight_dtype,
                                             const float* center, const float* height, const float* dim, const float* rot,
                                             const float* vel, const float* bbox_targets, const float* bbox_weights,
                                             const float* code_weights, const int* num_pos, const float* avg_cls, const float* avg_box,
                                             int B, int C, int L, int K, int D, double alpha, double gamma, float cls_weight,
                                             float box_weight, const float* grad_cls, const float* grad_box, float* grad_scores,
                                             float* grad_center, float* grad_height, float* grad_dim, float* grad_rot, float* grad_vel,
                                             void* stream);
int bevamd_centerhead_box_loss_forward(const float* const* maps, const long long* const* ind, const float* const* target,
                                       const unsigned char* const* mask, int num_tasks, int batch, int max_objs, long long hw,
                                       const float* code_weights, float loss_weight, float* loss, float* avg, void* stream);
int bevamd_centerhead_box_loss_backward(const float* const* maps, const long long* const* ind, const float* const* target,
                                        const unsigned char* const* mask, int num_tasks, int batch, int max_objs, long long hw,
                                        const float* code_weights, float loss_weight, const float* avg, const float* grad_out,
                                        float* const* grad_maps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVFUSION_AMD_EXT_H_ */
