// The rules behind ctk_fit_focal (include/ctk.h, "fit focal"), restated ONCE for the device kernels (focal.hip) and for a host build of the
// same text (tests/test_focal_host.py compiles this header with g++ and compares it with the numpy restatement of
// tests/focal_reference.py -- no GPU needed to pin it).  The header sits on top of pose_math.h and keeps its style: decisions are INTEGER
// or single comparisons; everything in double is ONE IEEE operation per step in the order written here (compile with
// -ffp-contract=off); no library root, logarithm or power; no sum depends on the order of accumulation: the device, the host build and
// numpy agree on every bit.  What is not named here is ctk_fit_pose's (pose_math.h): the fit list, the rays, E, the decomposition, the
// cheirality vote and the two Gauss-Newton rounds, all reused without change.
//
// Over a fit list there is one focal length at which a rigid pose explains the correspondences as well as the unconstrained
// fundamental matrix does.  K candidate focal lengths are swept through ctk_fit_pose's rules, each is scored in pixels, the scores are
// summed over frames in integers, and the smallest total is taken.
//   camera      of candidate k: fx = fy = focals[k] (float32, widened to double once), cx and cy the call's.  Square pixels only: the
//               score below is a pixel distance only then.  A candidate STANDS iff it is finite and > 0; one that does not sets bit 2.
//   takes part  a frame takes part iff its fit list has M >= min_points entries and ctk_pose_essential accepts its matrix under the
//               camera of at least one standing candidate.  A frame that does not take part costs 0 under every candidate and is
//               not counted.
//   fit         per (frame that takes part, candidate): ctk_fit_pose's rules under that camera -- ctk_pose_essential,
//               ctk_pose_decompose, the cheirality vote, CTK_POSE_ROUNDS rounds in which a failed round keeps its pose.
//   score       of a fit-list entry under the final pose: ctk_pose_entry gives v[6] = r and g.  If g > 0: r2 = r * r, q = r2 / g,
//               d2 = q * ff with ff = f * f (once per candidate), e = d2 / T with T = tol * tol in double (tol widened first);
//               c = e < 1 ? e : 1 (a NaN gives 1).  Otherwise c = 1.  With fx = fy = f the squared Sampson distance in pixels is
//               exactly f^2 r^2 / g.  term = llrint(c * 2^32): at most 2^32.
//   cost        cost[frame][k] = the int64 sum of the terms.  Where the candidate does not stand, ctk_pose_essential or
//               ctk_pose_decompose fails or no pose is left after the vote: M * 2^32, the largest sum there is.  At most 8192
//               entries a frame and 65535 frames a call (CTK_FOCAL_FRAMES_MAX): a call's sums stay below 2^32 * 2^13 * 2^16 = 2^61.
//   totals      total[k] = curve_in[k] + the sum of cost[frame][k] over the call's frames; the frames that took part and their entries
//               are carried alike in curve[K] and curve[K + 1].  (An accumulation over calls stays below 2^62 for 2^17 frames.)
//   choice      no fit when the counted frames < min_frames.  i = the smallest total, the lowest index on ties; mx = the largest.  No
//               fit, and bit 1, when !((double)mx >= contrast * (double)total[i]) -- one product, one comparison: the flat curve of a
//               camera that does not turn -- or when candidate i does not stand.
//   refine      0 < i < K - 1: a = (double)(total[i-1] - total[i]), d = (double)(total[i+1] - total[i]) (integer differences first),
//               den = a + d; den > 0: delta = (0.5 * (a - d)) / den, f = delta >= 0 ? f_i + delta * (f_{i+1} - f_i)
//               : f_i + delta * (f_i - f_{i-1}); otherwise, or where that neighbour does not stand, f = f_i.  i = 0 or i = K - 1: f = f_i and bit 0 (the range was too narrow).
//   outputs     focal = (float)f, 0.0f where there is no fit; stats = (frames counted, i or -1, entries counted, bits), the counts
//               clamped to int32.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pose_math.h"

#define CTK_FOCAL_K_MAX 256
#define CTK_FOCAL_FRAMES_MAX 65535
#define CTK_FOCAL_ONE 4294967296.0  // 2^32: the cost of an entry that is off by tol or more
#define CTK_FOCAL_BIT_END 1
#define CTK_FOCAL_BIT_FLAT 2
#define CTK_FOCAL_BIT_CANDIDATE 4

CTK_MM_HD bool ctk_focal_stands(float f) { return f > 0.0f && f <= 3.402823466e+38f; }

CTK_MM_HD CtkPoseCam ctk_focal_cam(float f, float cx, float cy) {
  CtkPoseCam k;
  k.fx = (double)f, k.fy = (double)f, k.cx = (double)cx, k.cy = (double)cy;
  return k;
}

// T of the score
CTK_MM_HD double ctk_focal_tol2(float tol) {
  const double t = (double)tol;
  return t * t;
}

// whether ctk_pose_essential accepts the matrix under candidate f
CTK_MM_HD bool ctk_focal_accepts(const float* F, float f, float cx, float cy) {
  if (!ctk_focal_stands(f)) return false;
  double E[9];
  return ctk_pose_essential(F, ctk_focal_cam(f, cx, cy), E);
}

// the term of one entry under the final pose; ff = f * f
CTK_MM_HD int64_t ctk_focal_term(const CtkPose& P, const double* x, const double* y, double ff, double T) {
  double v[7], g;
  (void)ctk_pose_entry(P, x, y, v, &g);
  double c = 1.0;
  if (g > 0.0) {
    const double r2 = v[6] * v[6];
    const double q = r2 / g;
    const double d2 = q * ff;
    const double e = d2 / T;
    c = e < 1.0 ? e : 1.0;
  }
  return (int64_t)llrint(c * CTK_FOCAL_ONE);
}

// the cost of a (frame, candidate) without a pose
CTK_MM_HD int64_t ctk_focal_worst(int M) { return (int64_t)M * 4294967296LL; }

CTK_MM_HD int32_t ctk_focal_clamp(int64_t v) { return v > 2147483647LL ? 2147483647 : (v < 0 ? 0 : (int32_t)v); }

// total[K]: the totals; frames: the frames counted, curve_in's included; bad: a candidate does not stand -> *focal, *index, the bits
CTK_MM_HD int ctk_focal_choose(const int64_t* total, const float* focals, int K, int64_t frames, int min_frames, float contrast, bool bad,
                               float* focal, int* index) {
  int bits = bad ? CTK_FOCAL_BIT_CANDIDATE : 0;
  *focal = 0.0f, *index = -1;
  if (frames < (int64_t)min_frames) return bits;
  int i = 0;
  int64_t mx = total[0];
  for (int k = 1; k < K; ++k) {
    if (total[k] < total[i]) i = k;
    if (total[k] > mx) mx = total[k];
  }
  const double lim = (double)contrast * (double)total[i];
  if (!((double)mx >= lim) || !ctk_focal_stands(focals[i])) return bits | CTK_FOCAL_BIT_FLAT;
  const double fi = (double)focals[i];
  double f = fi;
  if (i == 0 || i == K - 1) {
    bits |= CTK_FOCAL_BIT_END;
  } else {
    const double a = (double)(total[i - 1] - total[i]), d = (double)(total[i + 1] - total[i]);
    const double den = a + d;
    if (den > 0.0) {
      const double df = a - d;
      const double h = 0.5 * df;
      const double delta = h / den;
      const float nb = delta >= 0.0 ? focals[i + 1] : focals[i - 1];
      if (ctk_focal_stands(nb)) {
        const double step = delta >= 0.0 ? (double)nb - fi : fi - (double)nb;
        const double m = delta * step;
        f = fi + m;
      }
    }
  }
  *focal = (float)f, *index = i;
  return bits;
}
