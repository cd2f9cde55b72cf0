// Host build of co-tracker_amd/csrc/motion_math.h behind plain loops: the rules of ctk_fit_motion (include/ctk.h, "fit motion") without
// workgroups, LDS or a GPU (tests/test_motion_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/motion_math.h"

// -> valid; *p = 1/16 pixel (untouched when not valid)
extern "C" int host_motion_quant(float x, float s, int* p) { return ctk_motion_quant(x, s, p) ? 1 : 0; }

extern "C" int host_motion_tol(float tol) { return ctk_motion_tol(tol); }

extern "C" int64_t host_motion_base2(float min_base) { return ctk_motion_base2(min_base); }

extern "C" uint32_t host_motion_mix(uint32_t x) { return ctk_motion_mix(x); }

extern "C" void host_motion_sample(uint32_t seed, int f, int k, int M, int model, int* i, int* j) { ctk_motion_sample(seed, f, k, M, model, i, j); }

// The whole of ctk_fit_motion, one (group, frame) after the other; the arguments are the fields of ctk_fit_motion_args.
// -> 0, or -2 where T or base2 is refused
extern "C" int host_fit_motion(int G, int N, int N_out, int R, int f0, int F, int lag, int model, int K, uint32_t seed, float tol,
                               float min_base, float sx, float sy, float thresh, const float* hc, const uint8_t* visible, const float* hv,
                               const float* hf, const int32_t* first_row, float* motion, int8_t* inlier, int32_t* stats) {
  const int T = ctk_motion_tol(tol);
  const int64_t base2 = ctk_motion_base2(min_base);
  if (T == 0 || base2 < 0) return -2;
  struct Pt { int px, py, qx, qy, n; };
  std::vector<Pt> pts;
  for (long g = 0; g < G; ++g)
    for (int pic = 0; pic < F; ++pic) {
      const int f = f0 + pic, fs = f - lag;
      int8_t* inl = inlier + (g * F + pic) * (long)N_out;
      pts.clear();
      for (int n = 0; n < N_out; ++n) {
        inl[n] = -1;
        if (fs < 0) continue;
        if (first_row != nullptr && fs < first_row[g * N + n]) continue;
        const long rp = (g * R + fs % R) * N + n, rq = (g * R + f % R) * N + n;
        Pt t;
        t.n = n;
        if (!ctk_motion_quant(hc[rp * 2], sx, &t.px) || !ctk_motion_quant(hc[rp * 2 + 1], sy, &t.py)) continue;
        if (!ctk_motion_quant(hc[rq * 2], sx, &t.qx) || !ctk_motion_quant(hc[rq * 2 + 1], sy, &t.qy)) continue;
        const bool seen = visible != nullptr ? visible[rp] != 0 && visible[rq] != 0
                                             : ctk_draw_visible(hv[rp], hf[rp], thresh) && ctk_draw_visible(hv[rq], hf[rq], thresh);
        if (seen) pts.push_back(t);
      }
      const int M = (int)pts.size();
      int64_t best = -1;
      auto make = [&](int k, CtkMotionHyp* h) {
        int i, j;
        ctk_motion_sample(seed, f, k, M, model, &i, &j);
        return ctk_motion_hyp(model, pts[i].px, pts[i].py, pts[i].qx, pts[i].qy, pts[j].px, pts[j].py, pts[j].qx, pts[j].qy, T, base2, h);
      };
      if (M >= (model == CTK_MOTION_SIMILARITY ? 2 : 1))
        for (int k = 0; k < K; ++k) {
          CtkMotionHyp h;
          if (!make(k, &h)) continue;
          int count = 0;
          for (const Pt& t : pts) count += ctk_motion_inlier(model, h, t.px, t.py, t.qx, t.qy) ? 1 : 0;
          const int64_t key = ctk_motion_key(count, k, K);
          best = key > best ? key : best;
        }
      float* row = motion + (g * F + pic) * 6;
      int32_t* st = stats + (g * F + pic) * 4;
      st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
      if (best < 0) {
        ctk_motion_identity(row);
        for (const Pt& t : pts) inl[t.n] = 0;
        continue;
      }
      CtkMotionHyp hb;
      make(ctk_motion_key_k(best, K), &hb);
      int64_t s[CTK_MS_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (const Pt& t : pts) {
        const bool in = ctk_motion_inlier(model, hb, t.px, t.py, t.qx, t.qy);
        if (in) ctk_motion_accumulate(s, t.px, t.py, t.qx, t.qy);
        inl[t.n] = in ? 1 : 0;
      }
      ctk_motion_refit(model, s, row);
      st[1] = (int)s[CTK_MS_N], st[2] = ctk_motion_key_k(best, K);
    }
  return 0;
}
