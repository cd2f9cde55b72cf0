// The rules behind ctk_track_field and ctk_warp_field (include/ctk.h, "track field"), restated ONCE for the device kernels (field.hip)
// and for a host build of the same text (tests/test_field_host.py compiles this header with g++ into a program and compares it with the
// numpy restatement of tests/field_reference.py -- no GPU needed to pin it).  Everything past the quantisation of a position is INTEGER
// arithmetic except ONE IEEE double division per node component (compile with -ffp-contract=off): the device, the host build and numpy
// agree on every byte and every float bit.
//
// Field of frame f ("at") against a frame "to": on the picture grid of frame f, the displacement that leads to the matching position
// of frame "to" -- a picture known on frame "to" is warped BACKWARDS onto frame f.
//   position    ctk_motion_quant (motion_math.h): v = x * sx, valid iff finite and |v| <= 8192, P = (int)rintf(v * 16), 1/16 pixel.
//               P on frame f, Q on frame "to", d = Q - P                                                    |P| <= 2^17, |d| <= 2^18
//   to          a fixed frame to >= 0;  or f - lag, lag != 0 (a negative lag: forward flow);  or an anchor: positions and visibility
//               handed in, taken on frame anchor_frame
//   pair        slot n counts iff both frames are >= 0 and >= first_row[g, n] (the anchor's frame is anchor_frame), both positions are
//               valid and both are visible (ctk_draw_visible, draw_math.h: ctk_fit_motion's rule); M = the number of pairs
//   grid        cell c = 1 << cs (cs 2..6), gw = ((W - 1) >> cs) + 2 nodes across, node (i, j) at Nx = (i c) * 16 = i << (cs + 4)
//   weight      separable tent of R cells (R 1..4), rad = R c 16:  wx = max(0, 1024 - (|Px - Nx| * 1024) / rad), a floor division of
//               non-negatives; w = wx wy <= 2^20.  As rad = R << (cs + 4) and floor(a / (b k)) = floor(floor(a / b) / k), the quotient
//               is (|Px - Nx| << (6 - cs)) / R: a shift and a division by 1..4                     |Px - Nx| < 2^20: below 2^24
//   sums        per node Wn = sum w, Sx = sum w d.x, Sy = sum w d.y in int64: Wn <= 2^33, |S| <= 2^51 for 8192 pairs.  Integer sums: the
//               order of accumulation does not matter
//   pyramid     level l + 1 has ceil(h / 2) x ceil(w / 2) nodes, each the sum of its up-to-four children, up to 1 x 1; the levels lie
//               one after the other, three int64 (Wn, Sx, Sy) per node
//   value       node (i, j) takes the lowest level l at which node (j >> l, i >> l) has Wn >= 1:
//               F = (int32)llrint((double)(S * 16) / (double)Wn), 1/256 pixel, round half to even  (|S * 16| <= 2^55, |F| <= 2^22);
//               where even the 1 x 1 level is empty (M = 0, or every pair out of reach of every node) F = 0 and the level is 255
//
// Resampling through a field, output pixel (x, y):  i = x >> cs, ax = x & (c - 1); j, ay likewise (i + 1 <= gw - 1 by the grid rule)
//   D = (c - ax)(c - ay) F[j][i] + ax (c - ay) F[j][i+1] + (c - ax) ay F[j+1][i] + ax ay F[j+1][i+1] in int64 (|D| <= 2^12 * 2^31)
//   X = x * 256 + ((D + (c c >> 1)) >> 2 cs), an arithmetic shift (int64: a field handed in may hold any int32); ix = X >> 8, fx = X & 255
//   taps, borders and blend are ctk_warp_frames' (warp_math.h: ctk_warp_clamp, ctk_warp_blend); flow = (float)(X - x * 256) / 256.0f
#pragma once
#include <math.h>
#include <stdint.h>

#include "motion_math.h"  // ctk_motion_quant; draw_math.h: ctk_draw_visible
#include "warp_math.h"    // ctk_warp_clamp, ctk_warp_blend, CTK_WARP_FILL / CTK_WARP_EDGE

#if defined(__HIPCC__)
#define CTK_FM_HD __host__ __device__ __forceinline__
#else
#define CTK_FM_HD static inline
#endif

#define CTK_FIELD_POINTS_MAX 8192
#define CTK_FIELD_CS_MIN 2
#define CTK_FIELD_CS_MAX 6
#define CTK_FIELD_RADIUS_MAX 4
#define CTK_FIELD_NO_LEVEL 255

CTK_FM_HD int ctk_field_grid(int n, int cs) { return ((n - 1) >> cs) + 2; }

// the frame a field of frame f points to; < 0: none
CTK_FM_HD int ctk_field_to(int f, int to, int lag, bool anchored, int anchor_frame) { return anchored ? anchor_frame : (to >= 0 ? to : f - lag); }

// both positions of a slot -> valid; P (1/16 pixel) and d = Q - P
CTK_FM_HD bool ctk_field_pair(float px, float py, float qx, float qy, float sx, float sy, int* Px, int* Py, int* dx, int* dy) {
  int Qx = 0, Qy = 0;
  const bool ok0 = ctk_motion_quant(px, sx, Px), ok1 = ctk_motion_quant(py, sy, Py);
  const bool ok2 = ctk_motion_quant(qx, sx, &Qx), ok3 = ctk_motion_quant(qy, sy, &Qy);
  if (!(ok0 && ok1 && ok2 && ok3)) return false;
  *dx = Qx - *Px, *dy = Qy - *Py;
  return true;
}

// one axis of the tent: dist = |P - N| >= 0 in 1/16 pixel
CTK_FM_HD int ctk_field_tent(int dist, int cs, int R) {
  const int v = dist << (6 - cs);
  const int q = R == 1 ? v : (R == 2 ? v >> 1 : (R == 4 ? v >> 2 : v / 3));
  return q >= 1024 ? 0 : 1024 - q;
}

// the weight of a pair at (Px, Py) on the node at (Nx, Ny)
CTK_FM_HD int ctk_field_weight(int Px, int Py, int Nx, int Ny, int cs, int R) {
  const int ex = Px - Nx, ey = Py - Ny;
  return ctk_field_tent(ex < 0 ? -ex : ex, cs, R) * ctk_field_tent(ey < 0 ? -ey : ey, cs, R);
}

CTK_FM_HD void ctk_field_accumulate(int64_t* s, int w, int dx, int dy) {
  s[0] += (int64_t)w, s[1] += (int64_t)w * dx, s[2] += (int64_t)w * dy;
}

// nodes of all levels of a gh x gw grid
CTK_FM_HD int64_t ctk_field_nodes(int gh, int gw) {
  int64_t n = 0;
  for (int h = gh, w = gw;; h = (h + 1) >> 1, w = (w + 1) >> 1) {
    n += (int64_t)h * w;
    if (h == 1 && w == 1) return n;
  }
}

CTK_FM_HD int ctk_field_value(int64_t S, int64_t Wn) { return (int)llrint((double)(S * 16) / (double)Wn); }

// node (i, j) of a pyramid whose sums are complete -> its level; *fx, *fy = the value
CTK_FM_HD int ctk_field_resolve(const int64_t* pyr, int gh, int gw, int j, int i, int* fx, int* fy) {
  int64_t off = 0;
  for (int l = 0, h = gh, w = gw;; ++l) {
    const int64_t* e = pyr + (off + (int64_t)(j >> l) * w + (i >> l)) * 3;
    if (e[0] >= 1) {
      *fx = ctk_field_value(e[1], e[0]), *fy = ctk_field_value(e[2], e[0]);
      return l;
    }
    if (h == 1 && w == 1) break;
    off += (int64_t)h * w, h = (h + 1) >> 1, w = (w + 1) >> 1;
  }
  *fx = 0, *fy = 0;
  return CTK_FIELD_NO_LEVEL;
}

// one component of the four nodes round pixel offset (ax, ay) of a cell -> the displacement in 1/256 pixel
CTK_FM_HD int64_t ctk_field_sample(int f00, int f01, int f10, int f11, int ax, int ay, int cs) {
  const int c = 1 << cs;
  const int64_t D = (int64_t)((c - ax) * (c - ay)) * f00 + (int64_t)(ax * (c - ay)) * f01 + (int64_t)((c - ax) * ay) * f10 +
                    (int64_t)(ax * ay) * f11;
  return (D + ((c * c) >> 1)) >> (2 * cs);
}

CTK_FM_HD int64_t ctk_field_coord(int x, int64_t disp) { return (int64_t)x * 256 + disp; }
CTK_FM_HD int ctk_field_whole(int64_t X) { return (int)(X >> 8); }
CTK_FM_HD int ctk_field_frac(int64_t X) { return (int)(X & 255); }
CTK_FM_HD float ctk_field_flow(int64_t disp) { return (float)disp / 256.0f; }
