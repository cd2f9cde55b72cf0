// Host build of co-tracker_amd/csrc/epipolar_math.h behind plain loops: the rules of ctk_fit_epipolar (include/ctk.h, "fit epipolar")
// without workgroups, LDS or a GPU (tests/test_epipolar_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/epipolar_math.h"

extern "C" void host_epi_sample(uint32_t seed, int f, int k, int M, int* i) { ctk_epi_sample(seed, f, k, M, i); }

// pt: 32 ints, (Px, Py, Qx, Qy) of the eight sample points -> admissible; f: nine doubles; ej: the scale and j*
extern "C" int host_epi_hyp(const int* pt, int64_t base2, double* f, int* ej) {
  int q[8][4];
  for (int t = 0; t < 32; ++t) q[t / 4][t % 4] = pt[t];
  CtkEpiFit h;
  const bool ok = ctk_epi_hyp(q, base2, &h);
  for (int i = 0; i < 9; ++i) f[i] = h.f[i];
  ej[0] = h.e, ej[1] = h.jstar;
  return ok ? 1 : 0;
}

// The whole of ctk_fit_epipolar, one (group, frame) after the other; the arguments are the fields of ctk_fit_epipolar_args.
// -> 0, or -2 where T, base2 or min_points is refused
extern "C" int host_fit_epipolar(int G, int N, int N_out, int R, int f0, int F, int to, int lag, int anchor_frame, int min_points, int K,
                                 uint32_t seed, float tol, float min_base, float sx, float sy, float thresh, const float* hc,
                                 const uint8_t* visible, const float* hv, const float* hf, const int32_t* first_row, const float* ac,
                                 const uint8_t* av, const int8_t* mask, float* fundamental, int8_t* label, float* error, int32_t* stats) {
  const int Ti = ctk_motion_tol(tol);
  const int64_t base2 = ctk_motion_base2(min_base);
  if (Ti == 0 || base2 < 0 || min_points < CTK_EPI_MIN_POINTS) return -2;
  const double T = (double)Ti;
  struct Pt { int px, py, qx, qy, n; };
  std::vector<Pt> all, list;
  const bool anchored = ac != nullptr;
  for (long g = 0; g < G; ++g)
    for (int pic = 0; pic < F; ++pic) {
      const int f = f0 + pic, fs = ctk_objects_source(f, to, lag, anchored, anchor_frame);
      int8_t* lab = label + (g * F + pic) * (long)N_out;
      float* err = error + (g * F + pic) * (long)N_out;
      float* m9 = fundamental + (g * F + pic) * 9L;
      int32_t* st = stats + (g * F + pic) * 4L;
      all.clear(), list.clear();
      for (int n = 0; n < N_out; ++n) {
        lab[n] = -1, err[n] = -1.0f;
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
        lab[n] = 0;
        all.push_back(t);
        if (mask == nullptr || mask[g * N + n] != 0) list.push_back(t);
      }
      const int M = (int)list.size();
      for (int i = 0; i < 9; ++i) m9[i] = 0.0f;
      st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
      int64_t best = -1;
      auto make = [&](int k, CtkEpiFit* h) {
        int i[8], pt[8][4];
        ctk_epi_sample(seed, f, k, M, i);
        for (int t = 0; t < 8; ++t) pt[t][0] = list[i[t]].px, pt[t][1] = list[i[t]].py, pt[t][2] = list[i[t]].qx, pt[t][3] = list[i[t]].qy;
        return ctk_epi_hyp(pt, base2, h);
      };
      if (M >= CTK_EPI_SAMPLE)
        for (int k = 0; k < K; ++k) {
          CtkEpiFit h;
          if (!make(k, &h)) continue;
          int count = 0;
          for (const Pt& t : list) count += ctk_epi_inlier(h, T, t.px, t.py, t.qx, t.qy) ? 1 : 0;
          const int64_t key = ctk_motion_key(count, k, K);
          best = key > best ? key : best;
        }
      if (!ctk_objects_accept(best, min_points)) continue;
      CtkEpiFit cur;
      make(ctk_motion_key_k(best, K), &cur);
      int fell = 0;
      for (int round = 0; round < 2; ++round) {
        int reach = 0;
        for (const Pt& t : list)
          if (ctk_epi_inlier(cur, T, t.px, t.py, t.qx, t.qy)) {
            const int v = ctk_epi_reach(cur, t.px, t.py, t.qx, t.qy);
            reach = v > reach ? v : reach;
          }
        const int e = ctk_plane_bits(reach);
        int64_t s[CTK_EPI_SUMS];
        for (int i = 0; i < CTK_EPI_SUMS; ++i) s[i] = 0;
        // (backwards: the sums do not depend on the order of accumulation)
        for (size_t m = list.size(); m-- > 0;) {
          const Pt& t = list[m];
          if (ctk_epi_inlier(cur, T, t.px, t.py, t.qx, t.qy)) ctk_epi_terms(cur, e, t.px, t.py, t.qx, t.qy, s);
        }
        double work[64 + 8 + 64 + 8 + 8 + 8 + 8];
        const int jstar = round == 0 ? cur.jstar : ctk_epi_largest(cur.f, 9);
        CtkEpiFit next;
        if (ctk_epi_refit(cur, jstar, e, s, work, &next)) {
          cur = next;
        } else {
          fell |= 1 << round;
          if (round == 0) {
            ctk_epi_rescale(cur, e, &next);
            cur = next;
          }
        }
      }
      int count = 0;
      for (const Pt& t : list) count += ctk_epi_inlier(cur, T, t.px, t.py, t.qx, t.qy) ? 1 : 0;
      for (const Pt& t : all) {
        double r, gg;
        ctk_epi_residual(cur, t.px, t.py, t.qx, t.qy, &r, &gg);
        lab[t.n] = ctk_epi_test(r, gg, cur.e, T) ? 1 : 0;
        err[t.n] = ctk_epi_error(r, gg, cur.e);
      }
      ctk_epi_pixels(cur, m9);
      st[1] = count, st[2] = ctk_motion_key_k(best, K), st[3] = fell;
    }
  return 0;
}

// the error of one point from its (r, g) under a matrix of scale e
extern "C" float host_epi_error(double r, double g, int e) { return ctk_epi_error(r, g, e); }
