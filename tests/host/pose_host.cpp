// Host build of co-tracker_amd/csrc/pose_math.h behind plain loops: the rules of ctk_fit_pose (include/ctk.h, "fit pose") without
// workgroups, LDS or a GPU (tests/test_pose_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/pose_math.h"

extern "C" double host_pose_rsqrt(double a) { return ctk_pose_rsqrt(a); }

// R: nine doubles, orthogonalised in place -> the determinant
extern "C" double host_pose_polar(double* R) { return ctk_pose_polar(R); }

// F: nine floats; cam: fx, fy, cx, cy -> 0 no fit, 1 E only, 2 decomposed; E: nine doubles; cand: 4 x 12 doubles (R, t); ok: four ints
extern "C" int host_pose_decompose(const float* F, const float* cam, double* E, double* cand, int* ok) {
  const CtkPoseCam k = {(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3]};
  if (!ctk_pose_essential(F, k, E)) return 0;
  CtkPose c[4];
  bool o[4];
  const bool d = ctk_pose_decompose(E, c, o);
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 9; ++j) cand[i * 12 + j] = c[i].R[j];
    for (int j = 0; j < 3; ++j) cand[i * 12 + 9 + j] = c[i].t[j];
    ok[i] = o[i] ? 1 : 0;
  }
  return d ? 2 : 1;
}

// The whole of ctk_fit_pose, one (group, frame) after the other; the arguments are the fields of ctk_fit_pose_args.
// -> 0, or -2 where min_points is refused
extern "C" int host_fit_pose(int G, int N, int N_out, int R, int f0, int F, int to, int lag, int anchor_frame, int min_points, float fx,
                             float fy, float cx, float cy, float sx, float sy, float thresh, const float* hc, const uint8_t* visible,
                             const float* hv, const float* hf, const int32_t* first_row, const float* ac, const uint8_t* av,
                             const int8_t* mask, const float* fundamental, const int8_t* label, float* pose, float* depth, int32_t* stats) {
  if (min_points < CTK_POSE_MIN_POINTS || min_points > CTK_MOTION_POINTS_MAX) return -2;
  const CtkPoseCam cam = {(double)fx, (double)fy, (double)cx, (double)cy};
  struct Pt { int px, py, qx, qy, n; };
  std::vector<Pt> all, list;
  const bool anchored = ac != nullptr;
  for (long g = 0; g < G; ++g)
    for (int pic = 0; pic < F; ++pic) {
      const int f = f0 + pic, fs = ctk_objects_source(f, to, lag, anchored, anchor_frame);
      const long o = g * F + pic;
      const int8_t* lab = label + o * N_out;
      float* dep = depth + o * N_out * 2L;
      float* po = pose + o * 12L;
      int32_t* st = stats + o * 4L;
      all.clear(), list.clear();
      for (int n = 0; n < N_out; ++n) {
        dep[n * 2] = ctk_pose_nan(), dep[n * 2 + 1] = ctk_pose_nan();
        if (fs < 0) continue;
        if (first_row != nullptr && (fs < first_row[g * N + n] || f < first_row[g * N + n])) continue;
        const long rp = anchored ? g * N + n : (g * R + fs % R) * N + n, rq = (g * R + f % R) * N + n;
        const float* src = anchored ? ac : hc;
        Pt t;
        t.n = n;
        if (!ctk_motion_quant(src[rp * 2], sx, &t.px) || !ctk_motion_quant(src[rp * 2 + 1], sy, &t.py)) continue;
        if (!ctk_motion_quant(hc[rq * 2], sx, &t.qx) || !ctk_motion_quant(hc[rq * 2 + 1], sy, &t.qy)) continue;
        const bool vq = visible != nullptr ? visible[rq] != 0 : ctk_draw_visible(hv[rq], hf[rq], thresh);
        const bool vp = anchored ? av[rp] != 0 : (visible != nullptr ? visible[rp] != 0 : ctk_draw_visible(hv[rp], hf[rp], thresh));
        if (!(vp && vq)) continue;
        all.push_back(t);
        if (lab[n] == 1 && (mask == nullptr || mask[g * N + n] != 0)) list.push_back(t);
      }
      const int M = (int)list.size();
      ctk_pose_identity(po);
      st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
      double E[9];
      CtkPose cand[4];
      bool ok[4];
      if (!ctk_pose_essential(fundamental + o * 9L, cam, E) || M < min_points || !ctk_pose_decompose(E, cand, ok)) continue;
      auto rays = [&](const Pt& t, double* x, double* y) {
        ctk_pose_ray(cam, t.px, t.py, x);
        ctk_pose_ray(cam, t.qx, t.qy, y);
      };
      int count[4] = {0, 0, 0, 0};
      for (const Pt& t : list) {
        double x[3], y[3], zs, zf;
        rays(t, x, y);
        for (int k = 0; k < 4; ++k) {
          ctk_pose_depths(cand[k], x, y, &zs, &zf);
          count[k] += ctk_pose_front(zs, zf) ? 1 : 0;
        }
      }
      const int k = ctk_pose_choose(count, ok);
      if (k < 0) continue;
      CtkPose cur = cand[k];
      int bits = 0;
      for (int round = 0; round < CTK_POSE_ROUNDS; ++round) {
        int64_t s[CTK_POSE_SUMS];
        for (int i = 0; i < CTK_POSE_SUMS; ++i) s[i] = 0;
        int n = 0;
        // (backwards: the sums do not depend on the order of accumulation)
        for (size_t m = list.size(); m-- > 0;) {
          double x[3], y[3], v[7], gg;
          rays(list[m], x, y);
          if (ctk_pose_entry(cur, x, y, v, &gg)) {
            ctk_pose_terms(v, gg, s);
            ++n;
          }
        }
        if (n < M) bits |= 4;
        double work[CTK_POSE_SOLVE_DOUBLES];
        CtkPose next;
        if (ctk_pose_update(cur, s, n, work, &next)) cur = next;
        else bits |= 1 << round;
      }
      int front = 0;
      for (const Pt& t : list) {
        double x[3], y[3], zs, zf;
        rays(t, x, y);
        ctk_pose_depths(cur, x, y, &zs, &zf);
        front += ctk_pose_front(zs, zf) ? 1 : 0;
      }
      for (const Pt& t : all) {
        double x[3], y[3], zs, zf;
        rays(t, x, y);
        ctk_pose_depths(cur, x, y, &zs, &zf);
        dep[t.n * 2] = ctk_pose_depth_out(zs), dep[t.n * 2 + 1] = ctk_pose_depth_out(zf);
      }
      ctk_pose_out(cur, po);
      st[1] = front, st[2] = k, st[3] = bits;
    }
  return 0;
}
