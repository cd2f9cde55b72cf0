// Host build of co-tracker_amd/csrc/p3p_math.h behind plain loops: the rules of ctk_fit_p3p (include/ctk.h, "fit p3p") without
// workgroups, LDS or a GPU (tests/test_p3p_host.py).  Compile with -ffp-contract=off, like the device unit.  With -DP3P_HOST_MAIN the
// file is a stand-alone program that runs the same function on inputs it makes itself (a planted camera path, spoiled positions and
// structure points, collinear and repeated triples) and prints a checksum: what a sanitizer build of it runs.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/p3p_math.h"

// three entries (X: nine doubles, q: six integers) -> 1 and twelve doubles (R | t: nine of R, three of t), or 0 and (I, 0)
extern "C" int host_p3p_candidate(float fx, float fy, float cx, float cy, const double* X, const int* q, double* out) {
  const CtkPoseCam cam = {(double)fx, (double)fy, (double)cx, (double)cy};
  CtkPose p;
  const bool ok = ctk_p3p_candidate(cam, X, q, &p);
  for (int i = 0; i < 9; ++i) out[i] = p.R[i];
  for (int i = 0; i < 3; ++i) out[9 + i] = p.t[i];
  return ok ? 1 : 0;
}

// The whole of ctk_fit_p3p, one (group, frame) after the other; the arguments are the fields of ctk_fit_p3p_args.
// -> 0, or -2 where min_points, hypotheses or tol is refused
extern "C" int host_fit_p3p(int G, int N, int N_out, int R, int f0, int F, int to, int lag, int anchor_frame, int min_points,
                            int hypotheses, uint32_t seed, float fx, float fy, float cx, float cy, float sx, float sy, float thresh,
                            float tol, const float* hc, const uint8_t* visible, const float* hv, const float* hf,
                            const int32_t* first_row, const float* ac, const uint8_t* av, const float* structure, const int8_t* valid,
                            float* pose, int8_t* label, float* error, int32_t* stats) {
  if (min_points < CTK_RESECTION_MIN_POINTS || min_points > CTK_MOTION_POINTS_MAX) return -2;
  if (hypotheses < 1 || hypotheses > CTK_RESECTION_HYPOTHESES_MAX || !(tol > 0.0f) || !ctk_resection_finite32(tol)) return -2;
  const CtkPoseCam cam = {(double)fx, (double)fy, (double)cx, (double)cy};
  const double tol2 = ctk_resection_tol2(tol), c2 = ctk_resection_c2(cam), ic2 = ctk_resection_ic2(c2);
  const int K = hypotheses;
  struct Pt { int qx, qy, n; double X[3]; };
  std::vector<Pt> all;
  const bool anchored = ac != nullptr;
  for (long g = 0; g < G; ++g)
    for (int pic = 0; pic < F; ++pic) {
      const int f = f0 + pic, fs = ctk_objects_source(f, to, lag, anchored, anchor_frame);
      const long o = g * F + pic;
      int8_t* lab = label + o * N_out;
      float* err = error + o * N_out;
      float* po = pose + o * 12L;
      int32_t* st = stats + o * 4L;
      all.clear();
      int same = 0;
      for (int n = 0; n < N_out; ++n) {
        lab[n] = -1, err[n] = -1.0f;
        if (fs < 0) continue;
        if (first_row != nullptr && (fs < first_row[g * N + n] || f < first_row[g * N + n])) continue;
        const long rp = anchored ? g * N + n : (g * R + fs % R) * N + n, rq = (g * R + f % R) * N + n;
        const float* src = anchored ? ac : hc;
        Pt t;
        t.n = n;
        int px, py;
        if (!ctk_motion_quant(src[rp * 2], sx, &px) || !ctk_motion_quant(src[rp * 2 + 1], sy, &py)) continue;
        if (!ctk_motion_quant(hc[rq * 2], sx, &t.qx) || !ctk_motion_quant(hc[rq * 2 + 1], sy, &t.qy)) continue;
        const bool vq = visible != nullptr ? visible[rq] != 0 : ctk_draw_visible(hv[rq], hf[rq], thresh);
        const bool vp = anchored ? av[rp] != 0 : (visible != nullptr ? visible[rp] != 0 : ctk_draw_visible(hv[rp], hf[rp], thresh));
        if (!(vp && vq)) continue;
        if (!ctk_resection_point(structure + (g * N + n) * 3L, valid[g * N + n], t.X)) continue;
        lab[n] = 0;
        same += px == t.qx && py == t.qy ? 1 : 0;
        all.push_back(t);
      }
      const int A = (int)all.size(), M = A < CTK_RESECTION_LIST_MAX ? A : CTK_RESECTION_LIST_MAX;
      const bool still = A > 0 && same == A;
      int bits = (A > CTK_RESECTION_LIST_MAX ? CTK_RESECTION_BIT_CAP : 0) | (still ? CTK_RESECTION_BIT_STILL : 0);
      ctk_pose_identity(po);
      st[0] = M, st[1] = 0, st[2] = -1, st[3] = bits;
      if (M < min_points) continue;
      int best = -1, bk = -1;
      CtkPose cur;
      ctk_resection_eye(&cur);
      // (backwards: the winner does not depend on the order the candidates are made and scored in)
      for (int k = K; k >= (still ? K : 0); --k) {
        CtkPose c;
        ctk_resection_eye(&c);
        if (k < K) {
          int idx[4], q[6];
          double X[9];
          ctk_plane_sample(seed, f, k, M, idx);
          for (int i = 0; i < 3; ++i) {
            const Pt& t = all[idx[i]];
            X[i * 3] = t.X[0], X[i * 3 + 1] = t.X[1], X[i * 3 + 2] = t.X[2];
            q[i * 2] = t.qx, q[i * 2 + 1] = t.qy;
          }
          if (!ctk_p3p_candidate(cam, X, q, &c)) continue;
        }
        int cnt = 0;
        for (int m = 0; m < M; ++m) {
          double Xc[3], uvd[5];
          ctk_resection_apply(c, all[m].X, Xc);
          cnt += ctk_resection_within(ctk_resection_error(cam, Xc, all[m].qx, all[m].qy, uvd), tol2) ? 1 : 0;
        }
        if (bk < 0 || ctk_resection_better(cnt, k, best, bk)) best = cnt, bk = k, cur = c;
      }
      if (best < min_points) continue;
      for (int round = 0; round < CTK_RESECTION_ROUNDS && !still; ++round) {
        int64_t s[CTK_POSE_SUMS];
        for (int i = 0; i < CTK_POSE_SUMS; ++i) s[i] = 0;
        int n = 0;
        // (backwards: the sums do not depend on the order of accumulation)
        for (int m = M; m-- > 0;) {
          double Xc[3], uvd[5], vx[7], vy[7];
          ctk_resection_apply(cur, all[m].X, Xc);
          if (!ctk_resection_within(ctk_resection_error(cam, Xc, all[m].qx, all[m].qy, uvd), tol2)) continue;
          if (ctk_resection_entry(cam, c2, Xc, uvd, vx, vy)) {
            ctk_resection_terms(vy, ic2, s);
            ctk_resection_terms(vx, ic2, s);
            ++n;
          } else {
            bits |= 4;
          }
        }
        double work[CTK_POSE_SOLVE_DOUBLES];
        CtkPose next;
        if (ctk_resection_update(cur, s, n, work, &next)) cur = next;
        else bits |= round == 0 ? 1 : (round == 1 ? 2 : 16);
      }
      int ones = 0;
      for (const Pt& t : all) {
        double Xc[3], uvd[5];
        ctk_resection_apply(cur, t.X, Xc);
        const double e = ctk_resection_error(cam, Xc, t.qx, t.qy, uvd);
        lab[t.n] = ctk_resection_within(e, tol2) ? 1 : 0;
        err[t.n] = (float)e;
        ones += lab[t.n];
      }
      ctk_pose_out(cur, po);
      st[1] = ones, st[2] = bk, st[3] = bits;
    }
  return 0;
}

#ifdef P3P_HOST_MAIN
#include <stdio.h>

// A planted camera path over G groups, R ring rows and N points; positions, structure points and validity bytes are spoiled here and
// there (NaN, infinities, zero points, points behind the camera, a run of collinear points and a run of copies of one point); every
// source form is run once.
int main() {
  uint32_t lcg = 12345u;
  auto rnd = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (double)(lcg >> 8) / 16777216.0;
  };
  const float fx = 432.0f, fy = 430.0f, cx = 240.0f, cy = 135.0f;
  uint64_t sum = 0;
  int fitted = 0, rows = 0;
  for (int N : {6, 40, 257, 4200}) {
    const int G = 2, R = 6, F = 3, f0 = 7, N_out = N > 8 ? N - 1 : N;
    std::vector<float> hc((size_t)G * R * N * 2), str((size_t)G * N * 3), anchor((size_t)G * N * 2);
    std::vector<uint8_t> vis((size_t)G * R * N), av((size_t)G * N);
    std::vector<int8_t> valid((size_t)G * N);
    std::vector<int32_t> first((size_t)G * N, 0);
    for (int g = 0; g < G; ++g)
      for (int n = 0; n < N; ++n) {
        const double z = 3.0 + 9.0 * rnd(), x = (rnd() - 0.5) * z, y = (rnd() - 0.5) * 0.6 * z;
        float* s = &str[((size_t)g * N + n) * 3];
        s[0] = (float)x, s[1] = (float)y, s[2] = (float)z;
        valid[(size_t)g * N + n] = n % 11 == 3 ? 0 : (int8_t)(1 + n % 100);
        anchor[((size_t)g * N + n) * 2] = (float)(fx * x / z + cx), anchor[((size_t)g * N + n) * 2 + 1] = (float)(fy * y / z + cy);
        av[(size_t)g * N + n] = n % 17 != 2;
        if (n % 23 == 1) first[(size_t)g * N + n] = 8;
        for (int f = f0 - 3; f < f0 + F; ++f) {
          const double tx = 0.05 * (f - 4), tz = 0.01 * (f - 4);
          float* c = &hc[(((size_t)g * R + f % R) * N + n) * 2];
          c[0] = (float)(fx * (x + tx) / (z + tz) + cx + 0.1 * (rnd() - 0.5)), c[1] = (float)(fy * y / (z + tz) + cy + 0.1 * (rnd() - 0.5));
          if (n % 37 == 9) c[0] = n % 2 ? NAN : 1e9f;
          vis[((size_t)g * R + f % R) * N + n] = rnd() < 0.95;
        }
        // (the structure is spoiled after the positions were made from it)
        if (n % 29 == 5) s[n % 3] = n % 2 ? NAN : INFINITY;
        if (n % 31 == 7) s[2] = -s[2];
        if (n % 41 == 11) s[0] = s[1] = s[2] = 0.0f;
        if (n >= 20 && n < 26) s[0] = 0.25f * (n - 20), s[1] = 0.5f * (n - 20), s[2] = 4.0f + 0.125f * (n - 20);  // collinear
        if (n >= 30 && n < 34) s[0] = 1.0f, s[1] = -1.0f, s[2] = 5.0f;                                           // one point, four times
      }
    std::vector<float> pose((size_t)G * F * 12), err((size_t)G * F * N_out);
    std::vector<int8_t> lab((size_t)G * F * N_out);
    std::vector<int32_t> st((size_t)G * F * 4);
    for (int form = 0; form < 3; ++form) {
      const int rc = host_fit_p3p(G, N, N_out, R, f0, F, form == 1 ? 5 : -1, form == 0 ? 3 : 0, 4, 6, form == 2 ? 1024 : 33, 9u + form, fx, fy, cx, cy,
                                  1.0f, 1.0f, 0.5f, 2.0f, hc.data(), vis.data(), nullptr, nullptr, form == 2 ? first.data() : nullptr,
                                  form == 2 ? anchor.data() : nullptr, form == 2 ? av.data() : nullptr, str.data(), valid.data(), pose.data(),
                                  lab.data(), err.data(), st.data());
      if (rc != 0) return 2;
      for (size_t i = 0; i < st.size(); ++i) sum = sum * 31u + (uint32_t)st[i];
      for (size_t i = 0; i < lab.size(); ++i) sum = sum * 31u + (uint8_t)lab[i];
      for (size_t i = 0; i < pose.size(); ++i) {
        uint32_t b;
        __builtin_memcpy(&b, &pose[i], 4);
        sum = sum * 31u + b;
      }
      for (int i = 0; i < G * F; ++i) fitted += st[(size_t)i * 4 + 2] >= 0, ++rows;
    }
  }
  printf("p3p_host: %d of %d rows fitted, checksum %016llx\n", fitted, rows, (unsigned long long)sum);
  return fitted > 0 ? 0 : 3;
}
#endif
