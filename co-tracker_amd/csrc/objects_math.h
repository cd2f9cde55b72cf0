// The rules behind ctk_fit_objects (include/ctk.h, "fit objects"), restated ONCE for the device kernel (objects.hip) and for a host build
// of the same text (tests/test_objects_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/objects_reference.py -- no GPU needed to pin it).  Everything that is not named here is ctk_fit_motion's (motion_math.h), bit
// for bit: positions, mix, the sample, the hypothesis, inlier, key, refit.  Compile with -ffp-contract=off.
//
//   pair        P = source, Q = destination (frame f); the matrix maps the source frame onto frame f.  The source is exactly one of
//               ctk_track_field's three forms: a fixed frame to >= 0;  f - lag, lag >= 1;  an anchor (positions and visibility handed
//               in, taken on frame anchor_frame).  Slot n is a correspondence iff both frames are >= 0 and >= first_row[g, n] (the
//               anchor's frame is anchor_frame), both positions are valid and both are visible.  The M correspondences are numbered in
//               ascending n.
//   rounds      r = 0 .. L - 1, L in 1..16.  Round r fits list_r, a sub-list of the correspondences in ascending n with M_r entries:
//               labels mode   list_r = the correspondences whose label is r; a label outside 0..L-1 belongs to no round
//               split mode    list_0 = all correspondences; list_{r+1} = list_r without the inliers of round r's best hypothesis
//               The sample of round r uses seed_r = seed ^ mix(r) (mix(0) = 0: round 0 uses seed itself); otherwise the round is
//               ctk_fit_motion's hypothesis, scoring, best and refit over list_r, with f the absolute frame number.
//   acceptance  a round whose best has fewer than min_points (1..8192) inliers, or no admissible hypothesis, fits nothing: the
//               identity, stats (M_r, 0, -1, 0), box (0, 0, -1, -1), none of its points taken.  In split mode it ends the rounds:
//               every later round reports the same M_r and nothing else.  In labels mode the rounds are independent.
//   box         (min Qx, min Qy, max Qx, max Qy) over the round's inliers, 1/16 pixel
//   label       per slot: -1 no correspondence; r = inlier of round r's accepted best; CTK_OBJECT_NONE = a correspondence no round took
#pragma once
#include <stdint.h>

#include "motion_math.h"

#define CTK_OBJECTS_MAX 16
#define CTK_OBJECT_NONE 127

// the seed of round r
CTK_MM_HD uint32_t ctk_objects_seed(uint32_t seed, int r) { return seed ^ ctk_motion_mix((uint32_t)r); }

// the source frame of frame f; < 0: none
CTK_MM_HD int ctk_objects_source(int f, int to, int lag, bool anchored, int anchor_frame) { return anchored ? anchor_frame : (to >= 0 ? to : f - lag); }

// the round a label belongs to; -1: none
CTK_MM_HD int ctk_objects_round(int label, int L) { return label >= 0 && label < L ? label : -1; }

// is the best of a round (a key, -1 = no admissible hypothesis) a fit?
CTK_MM_HD bool ctk_objects_accept(int64_t best, int min_points) { return best >= 0 && ctk_motion_key_count(best) >= min_points; }

// the box of a round's inliers: starts empty, grows by one destination
CTK_MM_HD void ctk_objects_box_empty(int* b) { b[0] = INT32_MAX, b[1] = INT32_MAX, b[2] = INT32_MIN, b[3] = INT32_MIN; }
CTK_MM_HD void ctk_objects_box_add(int* b, int qx, int qy) {
  b[0] = qx < b[0] ? qx : b[0], b[1] = qy < b[1] ? qy : b[1];
  b[2] = qx > b[2] ? qx : b[2], b[3] = qy > b[3] ? qy : b[3];
}
// what a round that fits nothing reports
CTK_MM_HD void ctk_objects_box_none(int* b) { b[0] = 0, b[1] = 0, b[2] = -1, b[3] = -1; }
