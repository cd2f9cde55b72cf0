// Host build of co-tracker_amd/csrc/objects_math.h behind plain loops: the rules of ctk_fit_objects (include/ctk.h, "fit objects") without
// workgroups, LDS or a GPU (tests/test_objects_host.py).  Compile with -ffp-contract=off, like the device unit.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/objects_math.h"

extern "C" uint32_t host_objects_seed(uint32_t seed, int r) { return ctk_objects_seed(seed, r); }

extern "C" int host_objects_source(int f, int to, int lag, int anchored, int anchor_frame) {
  return ctk_objects_source(f, to, lag, anchored != 0, anchor_frame);
}

extern "C" int host_objects_round(int label, int L) { return ctk_objects_round(label, L); }

// The whole of ctk_fit_objects, one (group, frame) after the other; the arguments are the fields of ctk_fit_objects_args.
// -> 0, or -2 where T or base2 is refused
extern "C" int host_fit_objects(int G, int N, int N_out, int R, int f0, int F, int to, int lag, int anchor_frame, int L, int min_points,
                                int model, int K, uint32_t seed, float tol, float min_base, float sx, float sy, float thresh,
                                const float* hc, const uint8_t* visible, const float* hv, const float* hf, const int32_t* first_row,
                                const float* ac, const uint8_t* av, const int8_t* labels, float* motion, int8_t* label, int32_t* stats,
                                int32_t* box) {
  const int T = ctk_motion_tol(tol);
  const int64_t base2 = ctk_motion_base2(min_base);
  if (T == 0 || base2 < 0) return -2;
  struct Pt { int px, py, qx, qy, n; };
  std::vector<Pt> all, list, rest;
  const bool anchored = ac != nullptr;
  for (long g = 0; g < G; ++g)
    for (int pic = 0; pic < F; ++pic) {
      const int f = f0 + pic, fs = ctk_objects_source(f, to, lag, anchored, anchor_frame);
      int8_t* lab = label + (g * F + pic) * (long)N_out;
      all.clear();
      for (int n = 0; n < N_out; ++n) {
        lab[n] = -1;
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
        lab[n] = CTK_OBJECT_NONE;
        all.push_back(t);
      }
      if (labels == nullptr) list = all;
      bool stopped = false;
      for (int r = 0; r < L; ++r) {
        if (labels != nullptr) {
          list.clear();
          for (const Pt& t : all)
            if (ctk_objects_round(labels[g * N + t.n], L) == r) list.push_back(t);
        }
        const long o = (g * F + pic) * (long)L + r;
        float* row = motion + o * 6;
        int32_t* st = stats + o * 4;
        int32_t* bo = box + o * 4;
        const int M = (int)list.size();
        ctk_motion_identity(row);
        st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
        ctk_objects_box_none(bo);
        if (stopped) continue;
        const uint32_t seed_r = ctk_objects_seed(seed, r);
        int64_t best = -1;
        auto make = [&](int k, CtkMotionHyp* h) {
          int i, j;
          ctk_motion_sample(seed_r, f, k, M, model, &i, &j);
          return ctk_motion_hyp(model, list[i].px, list[i].py, list[i].qx, list[i].qy, list[j].px, list[j].py, list[j].qx, list[j].qy, T, base2,
                                h);
        };
        if (M >= (model == CTK_MOTION_SIMILARITY ? 2 : 1))
          for (int k = 0; k < K; ++k) {
            CtkMotionHyp h;
            if (!make(k, &h)) continue;
            int count = 0;
            for (const Pt& t : list) count += ctk_motion_inlier(model, h, t.px, t.py, t.qx, t.qy) ? 1 : 0;
            const int64_t key = ctk_motion_key(count, k, K);
            best = key > best ? key : best;
          }
        if (!ctk_objects_accept(best, min_points)) {
          stopped = labels == nullptr;
          continue;
        }
        CtkMotionHyp hb;
        make(ctk_motion_key_k(best, K), &hb);
        int64_t s[CTK_MS_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
        int b[4];
        ctk_objects_box_empty(b);
        rest.clear();
        for (const Pt& t : list) {
          if (ctk_motion_inlier(model, hb, t.px, t.py, t.qx, t.qy)) {
            ctk_motion_accumulate(s, t.px, t.py, t.qx, t.qy);
            ctk_objects_box_add(b, t.qx, t.qy);
            lab[t.n] = (int8_t)r;
          } else {
            rest.push_back(t);
          }
        }
        ctk_motion_refit(model, s, row);
        st[1] = (int)s[CTK_MS_N], st[2] = ctk_motion_key_k(best, K);
        bo[0] = b[0], bo[1] = b[1], bo[2] = b[2], bo[3] = b[3];
        if (labels == nullptr) list = rest;
      }
    }
  return 0;
}
