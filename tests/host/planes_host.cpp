// Host build of co-tracker_amd/csrc/plane_math.h behind plain loops: the rules of ctk_fit_planes and ctk_warp_planes (include/ctk.h,
// "fit planes / warp planes") without workgroups, LDS or a GPU (tests/test_planes_host.py).  Compile with -ffp-contract=off, like the
// device units.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/plane_math.h"

extern "C" void host_plane_sample(uint32_t seed, int f, int k, int M, int* i) { ctk_plane_sample(seed, f, k, M, i); }

// pt: 16 ints, (Px, Py, Qx, Qy) of the four sample points -> admissible; h: nine doubles
extern "C" int host_plane_hyp(const int* pt, int64_t base2, double* h) {
  int q[4][4];
  for (int t = 0; t < 16; ++t) q[t / 4][t % 4] = pt[t];
  CtkPlaneHyp hy;
  const bool ok = ctk_plane_hyp(q, base2, &hy);
  for (int i = 0; i < 9; ++i) h[i] = hy.h[i];
  return ok ? 1 : 0;
}

// The whole of ctk_fit_planes, one (group, frame) after the other; the arguments are the fields of ctk_fit_planes_args.
// -> 0, or -2 where T or base2 is refused
extern "C" int host_fit_planes(int G, int N, int N_out, int R, int f0, int F, int to, int lag, int anchor_frame, int L, int min_points,
                               int inverse, int K, uint32_t seed, float tol, float min_base, float sx, float sy, float thresh,
                               const float* hc, const uint8_t* visible, const float* hv, const float* hf, const int32_t* first_row,
                               const float* ac, const uint8_t* av, const int8_t* labels, float* homography, int8_t* label, int32_t* stats,
                               int32_t* box) {
  const int Ti = ctk_motion_tol(tol);
  const int64_t base2 = ctk_motion_base2(min_base);
  if (Ti == 0 || base2 < 0) return -2;
  const double T = (double)Ti;
  struct Pt { int px, py, qx, qy, n; };
  std::vector<Pt> all, list;
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
        if (inverse) {
          const Pt s = t;
          t.px = s.qx, t.py = s.qy, t.qx = s.px, t.qy = s.py;
        }
        lab[n] = CTK_OBJECT_NONE;
        all.push_back(t);
      }
      for (int r = 0; r < L; ++r) {
        list.clear();
        for (const Pt& t : all)
          if ((labels != nullptr ? ctk_objects_round(labels[g * N + t.n], L) : 0) == r) list.push_back(t);
        const long o = (g * F + pic) * (long)L + r;
        float* m9 = homography + o * 9;
        int32_t* st = stats + o * 4;
        int32_t* bo = box + o * 4;
        const int M = (int)list.size();
        ctk_plane_identity(m9);
        st[0] = M, st[1] = 0, st[2] = -1, st[3] = 0;
        ctk_objects_box_none(bo);
        const uint32_t seed_r = ctk_objects_seed(seed, r);
        int64_t best = -1;
        auto make = [&](int k, CtkPlaneHyp* h) {
          int i[4], pt[4][4];
          ctk_plane_sample(seed_r, f, k, M, i);
          for (int t = 0; t < 4; ++t) pt[t][0] = list[i[t]].px, pt[t][1] = list[i[t]].py, pt[t][2] = list[i[t]].qx, pt[t][3] = list[i[t]].qy;
          return ctk_plane_hyp(pt, base2, h);
        };
        if (M >= 4)
          for (int k = 0; k < K; ++k) {
            CtkPlaneHyp h;
            if (!make(k, &h)) continue;
            int count = 0;
            for (const Pt& t : list) count += ctk_plane_inlier(h, T, t.px, t.py, t.qx, t.qy) ? 1 : 0;
            const int64_t key = ctk_motion_key(count, k, K);
            best = key > best ? key : best;
          }
        if (!ctk_objects_accept(best, min_points)) continue;
        CtkPlaneHyp hb;
        make(ctk_motion_key_k(best, K), &hb);
        int reach = 0;
        for (const Pt& t : list)
          if (ctk_plane_inlier(hb, T, t.px, t.py, t.qx, t.qy)) {
            const int v = ctk_plane_reach(hb, t.px, t.py, t.qx, t.qy);
            reach = v > reach ? v : reach;
          }
        const int e = ctk_plane_bits(reach);
        int64_t s[CTK_PS_COUNT];
        for (int i = 0; i < CTK_PS_COUNT; ++i) s[i] = 0;
        int b[4];
        ctk_objects_box_empty(b);
        // (backwards: the sums do not depend on the order of accumulation)
        for (size_t m = list.size(); m-- > 0;) {
          const Pt& t = list[m];
          if (!ctk_plane_inlier(hb, T, t.px, t.py, t.qx, t.qy)) continue;
          ctk_plane_terms(hb, e, t.px, t.py, t.qx, t.qy, s);
          if (inverse) ctk_objects_box_add(b, t.px, t.py);
          else ctk_objects_box_add(b, t.qx, t.qy);
          lab[t.n] = (int8_t)r;
        }
        double Nm[64], bv[8], Lm[64], Dv[8], vv[8], zv[8], hv8[8], hc9[9];
        ctk_plane_system(s, Nm, bv);
        if (ctk_plane_solve(Nm, bv, Lm, Dv, vv, zv, hv8)) {
          for (int i = 0; i < 8; ++i) hc9[i] = hv8[i];
          hc9[8] = 1.0;
          ctk_plane_pixels(hc9, e, hb.px, hb.py, hb.qx, hb.qy, m9);
        } else {
          st[3] = 1;
          ctk_plane_pixels(hb.h, 0, hb.px, hb.py, hb.qx, hb.qy, m9);
        }
        st[1] = ctk_motion_key_count(best), st[2] = ctk_motion_key_k(best, K);
        bo[0] = b[0], bo[1] = b[1], bo[2] = b[2], bo[3] = b[3];
      }
    }
  return 0;
}

// The coordinate rule of ctk_warp_planes over an H x W output: inside [H,W] (0 / 1), X, Y [H,W] in 1/256 pixel (0 where outside)
extern "C" void host_warp_coords(const float* m, int H, int W, uint8_t* inside, int64_t* X, int64_t* Y) {
  double md[9];
  const bool finite = ctk_plane_matrix(m, md);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int64_t cx = 0, cy = 0;
      const bool in = finite && ctk_plane_coord(md, x, y, &cx, &cy);
      inside[(long)y * W + x] = in ? 1 : 0;
      X[(long)y * W + x] = in ? cx : 0, Y[(long)y * W + x] = in ? cy : 0;
    }
}

// ctk_warp_planes on channels-last pictures: dst (H x W x C) holds what is there before the call
extern "C" void host_warp_planes(const uint8_t* src, int Hs, int Ws, int C, const float* m, int border, const uint8_t* fill, uint8_t* dst, int H,
                                 int W) {
  double md[9];
  const bool finite = ctk_plane_matrix(m, md);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t* out = dst + ((long)y * W + x) * C;
      int64_t X = 0, Y = 0;
      if (!(finite && ctk_plane_coord(md, x, y, &X, &Y))) {
        if (border != CTK_WARP_KEEP)
          for (int ch = 0; ch < C; ++ch) out[ch] = fill[ch];
        continue;
      }
      const int ix = ctk_plane_whole(X), iy = ctk_plane_whole(Y), fx = ctk_plane_frac(X), fy = ctk_plane_frac(Y);
      const int x0 = ctk_warp_clamp(ix, Ws), x1 = ctk_warp_clamp(ix + 1, Ws), y0 = ctk_warp_clamp(iy, Hs), y1 = ctk_warp_clamp(iy + 1, Hs);
      const bool inx0 = x0 == ix, inx1 = x1 == ix + 1, iny0 = y0 == iy, iny1 = y1 == iy + 1;
      if (border == CTK_WARP_KEEP && !(inx0 && inx1 && iny0 && iny1)) continue;
      for (int ch = 0; ch < C; ++ch) {
        int p00 = src[((long)y0 * Ws + x0) * C + ch], p01 = src[((long)y0 * Ws + x1) * C + ch];
        int p10 = src[((long)y1 * Ws + x0) * C + ch], p11 = src[((long)y1 * Ws + x1) * C + ch];
        if (border == CTK_WARP_FILL) {
          const int fv = fill[ch];
          p00 = inx0 && iny0 ? p00 : fv, p01 = inx1 && iny0 ? p01 : fv, p10 = inx0 && iny1 ? p10 : fv, p11 = inx1 && iny1 ? p11 : fv;
        }
        out[ch] = (uint8_t)ctk_warp_blend(fx, fy, p00, p01, p10, p11);
      }
    }
}
