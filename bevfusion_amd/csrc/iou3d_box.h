// Rotated-box BEV overlap arithmetic shared by csrc/iou3d.hip (pairwise IoU, NMS mask), csrc/ext/centerpoint_ends.hip (the
// segmented rotated NMS of CenterHead) and csrc/ext/head_assign.hip (the IoU of the match cost): one box's derived values, the
// reference's polygon-of-crossings overlap and the IoU (iou3d_kernel.cu:126-229).  Device code only.
//
// Every function opens with `#pragma clang fp contract(off)`: products and sums round separately, wherever a unit includes the
// header.  The algorithm decides by the SIGN of differences of products (the strict straddle test s1 * s2 > 0 && s3 * s4 > 0, the
// |s5 - s1| > EPS split) and on collinear edges those differences are exact zeros only when both products round alike.  Fused, one
// product keeps its low bits and such a zero becomes a tiny number of either sign, so the tests can see crossings that are not
// there.  Measured on an MI355X under the default contraction: boxes of equal size and yaw slid along their own axis came out up
// to 0.12 off in IoU (6 of 1024 pairs), and the same rectangle written as (l, w, yaw + pi / 2) once came out as 7e9.  Un-fused,
// the device's error against float64 equals the fp32 CPU restatement's to two digits on every family of tests/iou3d_families.py
// (profiles/iou3d_families_parity_observed.json).  The pragma covers make_box, the centroid / atan2 keys and iou_rotated too, not
// only the sign tests: the corners those tests read come from make_box's rotation, the CPU restatement that every bar and golden
// keep set is stated against is built without contraction as a whole, and one rule for the header is what lets three units
// include it anywhere.  What is left is the reference's own: on about 0.05 % of near-duplicate pairs the algorithm itself
// returns finite, positive, meaningless values.
#pragma once

#include "common.h"

namespace bevamd {
namespace iou3d {

constexpr float EPS = 1e-8f;
struct Pt { float x, y; };

__device__ __forceinline__ float cross3(Pt p1, Pt p2, Pt p0) {
#pragma clang fp contract(off)
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// everything that depends on one box only
struct Box {
  float x1, y1, x2, y2;
  float cin, sin_;  // cos(-angle), sin(-angle): rotation used by the containment test
  Pt c[5];          // corners rotated by +angle about the centre, c[4] = c[0]
};

__device__ __forceinline__ Box make_box(const float* __restrict__ b) {
#pragma clang fp contract(off)
  Box r;
  r.x1 = b[0]; r.y1 = b[1]; r.x2 = b[2]; r.y2 = b[3];
  const float ang = b[4];
  const float cx = (r.x1 + r.x2) / 2, cy = (r.y1 + r.y2) / 2;
  const float co = cosf(ang), si = sinf(ang);
  r.cin = cosf(-ang);
  r.sin_ = sinf(-ang);
  const float px[4] = {r.x1, r.x2, r.x2, r.x1}, py[4] = {r.y1, r.y1, r.y2, r.y2};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r.c[k].x = (px[k] - cx) * co + (py[k] - cy) * si + cx;
    r.c[k].y = -(px[k] - cx) * si + (py[k] - cy) * co + cy;
  }
  r.c[4] = r.c[0];
  return r;
}

__device__ __forceinline__ bool contains(const Box& b, Pt p) {
#pragma clang fp contract(off)
  const float MARGIN = 1e-5f;
  const float cx = (b.x1 + b.x2) / 2, cy = (b.y1 + b.y2) / 2;
  const float rx = (p.x - cx) * b.cin + (p.y - cy) * b.sin_ + cx;
  const float ry = -(p.x - cx) * b.sin_ + (p.y - cy) * b.cin + cy;
  return rx > b.x1 - MARGIN && rx < b.x2 + MARGIN && ry > b.y1 - MARGIN && ry < b.y2 + MARGIN;
}

__device__ __forceinline__ bool seg_intersection(Pt p1, Pt p0, Pt q1, Pt q0, Pt& ans) {
#pragma clang fp contract(off)
  const bool rect = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                    fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
  if (!rect) return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > EPS) {
    ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    ans.x = (b0 * c1 - b1 * c0) / D;
    ans.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

__device__ float overlap(const Box& A, const Box& B) {
#pragma clang fp contract(off)
  Pt poly[16];
  float key[16];
  int cnt = 0;
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Pt p;
      if (seg_intersection(A.c[i + 1], A.c[i], B.c[j + 1], B.c[j], p)) {
        sx += p.x;
        sy += p.y;
        poly[cnt++] = p;
      }
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (contains(A, B.c[k])) {
      sx += B.c[k].x;
      sy += B.c[k].y;
      poly[cnt++] = B.c[k];
    }
    if (contains(B, A.c[k])) {
      sx += A.c[k].x;
      sy += A.c[k].y;
      poly[cnt++] = A.c[k];
    }
  }
  if (cnt < 3) return 0.f;  // the reference's loops produce area 0 here as well
  const float cx = sx / cnt, cy = sy / cnt;
  for (int i = 0; i < cnt; ++i) key[i] = atan2f(poly[i].y - cy, poly[i].x - cx);
  // the reference bubble-sorts with a strict '>' comparison on the same keys: a stable ascending sort
  for (int j = 0; j < cnt - 1; ++j)
    for (int i = 0; i < cnt - j - 1; ++i)
      if (key[i] > key[i + 1]) {
        const Pt tp = poly[i];
        poly[i] = poly[i + 1];
        poly[i + 1] = tp;
        const float tk = key[i];
        key[i] = key[i + 1];
        key[i + 1] = tk;
      }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; ++k) {
    const float ux = poly[k].x - poly[0].x, uy = poly[k].y - poly[0].y;
    const float vx = poly[k + 1].x - poly[0].x, vy = poly[k + 1].y - poly[0].y;
    area += ux * vy - uy * vx;
  }
  return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_rotated(const Box& A, const Box& B) {
#pragma clang fp contract(off)
  const float sa = (A.x2 - A.x1) * (A.y2 - A.y1), sb = (B.x2 - B.x1) * (B.y2 - B.y1);
  const float so = overlap(A, B);
  return so / fmaxf(sa + sb - so, EPS);
}

}  // namespace iou3d
}  // namespace bevamd
