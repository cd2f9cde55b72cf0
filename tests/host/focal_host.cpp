// Host build of co-tracker_amd/csrc/focal_math.h behind plain loops: the rules of ctk_fit_focal (include/ctk.h, "fit focal") without
// workgroups, LDS or a GPU (tests/test_focal_host.py).  Compile with -ffp-contract=off, like the device unit.  With -DFOCAL_HOST_MAIN the
// file is a stand-alone program that runs the same function on inputs it makes itself and prints a checksum: what a sanitizer build of
// it runs.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/focal_math.h"

namespace {
struct Pt { int px, py, qx, qy; };

// the pose of ctk_fit_pose's rules over the list under cam -> a pose stands
bool pose_of(const std::vector<Pt>& list, const float* Fm, const CtkPoseCam& cam, CtkPose* out) {
  double E[9];
  CtkPose cand[4];
  bool ok[4];
  if (!ctk_pose_essential(Fm, cam, E) || !ctk_pose_decompose(E, cand, ok)) return false;
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
  if (k < 0) return false;
  CtkPose cur = cand[k];
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
    double work[CTK_POSE_SOLVE_DOUBLES];
    CtkPose next;
    if (ctk_pose_update(cur, s, n, work, &next)) cur = next;
  }
  *out = cur;
  return true;
}
}  // namespace

// The whole of ctk_fit_focal, one group after the other; the arguments are the fields of ctk_fit_focal_args.
// -> 0, or -2 where a number is refused
extern "C" int host_fit_focal(int G, int N, int N_out, int R, int f0, int F, int to, int lag, int anchor_frame, int min_points, int K,
                              int min_frames, float cx, float cy, float sx, float sy, float thresh, float tol, float contrast,
                              const float* hc, const uint8_t* visible, const float* hv, const float* hf, const int32_t* first_row,
                              const float* ac, const uint8_t* av, const int8_t* mask, const float* fundamental, const int8_t* label,
                              const float* focals, const int64_t* curve_in, float* focal, int64_t* curve, int64_t* cost, int32_t* stats) {
  if (min_points < CTK_POSE_MIN_POINTS || min_points > CTK_MOTION_POINTS_MAX || K < 1 || K > CTK_FOCAL_K_MAX || min_frames < 1 ||
      F > CTK_FOCAL_FRAMES_MAX || !(contrast >= 1.0f))
    return -2;
  std::vector<Pt> list;
  std::vector<int64_t> total(K);
  const bool anchored = ac != nullptr;
  const double T = ctk_focal_tol2(tol);
  bool bad = false;
  for (int k = 0; k < K; ++k) bad = bad || !ctk_focal_stands(focals[k]);
  for (long g = 0; g < G; ++g) {
    const int64_t* in = curve_in != nullptr ? curve_in + g * (K + 2) : nullptr;
    for (int k = 0; k < K; ++k) total[k] = in != nullptr ? in[k] : 0;
    int64_t frames = in != nullptr ? in[K] : 0, entries = in != nullptr ? in[K + 1] : 0;
    for (int pic = 0; pic < F; ++pic) {
      const int f = f0 + pic, fs = ctk_objects_source(f, to, lag, anchored, anchor_frame);
      const long o = g * F + pic;
      const int8_t* lab = label + o * N_out;
      const float* Fm = fundamental + o * 9L;
      int64_t* co = cost + o * K;
      list.clear();
      for (int n = 0; n < N_out && fs >= 0; ++n) {
        if (first_row != nullptr && (fs < first_row[g * N + n] || f < first_row[g * N + n])) continue;
        const long rp = anchored ? g * N + n : (g * R + fs % R) * N + n, rq = (g * R + f % R) * N + n;
        const float* src = anchored ? ac : hc;
        Pt t;
        if (!ctk_motion_quant(src[rp * 2], sx, &t.px) || !ctk_motion_quant(src[rp * 2 + 1], sy, &t.py)) continue;
        if (!ctk_motion_quant(hc[rq * 2], sx, &t.qx) || !ctk_motion_quant(hc[rq * 2 + 1], sy, &t.qy)) continue;
        const bool vq = visible != nullptr ? visible[rq] != 0 : ctk_draw_visible(hv[rq], hf[rq], thresh);
        const bool vp = anchored ? av[rp] != 0 : (visible != nullptr ? visible[rp] != 0 : ctk_draw_visible(hv[rp], hf[rp], thresh));
        if (!(vp && vq)) continue;
        if (lab[n] == 1 && (mask == nullptr || mask[g * N + n] != 0)) list.push_back(t);
      }
      const int M = (int)list.size();
      bool any = false;
      for (int k = 0; k < K; ++k) any = any || ctk_focal_accepts(Fm, focals[k], cx, cy);
      const bool takes = M >= min_points && any;
      for (int k = 0; k < K; ++k) {
        int64_t sum = 0;
        if (takes) {
          sum = ctk_focal_worst(M);
          const CtkPoseCam cam = ctk_focal_cam(focals[k], cx, cy);
          CtkPose fin;
          if (ctk_focal_stands(focals[k]) && pose_of(list, Fm, cam, &fin)) {
            const double fd = (double)focals[k];
            const double ff = fd * fd;
            sum = 0;
            for (const Pt& t : list) {
              double x[3], y[3];
              ctk_pose_ray(cam, t.px, t.py, x);
              ctk_pose_ray(cam, t.qx, t.qy, y);
              sum += ctk_focal_term(fin, x, y, ff, T);
            }
          }
        }
        co[k] = sum, total[k] += sum;
      }
      frames += takes ? 1 : 0, entries += takes ? M : 0;
    }
    int index;
    const int bits = ctk_focal_choose(total.data(), focals, K, frames, min_frames, contrast, bad, focal + g, &index);
    int64_t* cu = curve + g * (K + 2);
    for (int k = 0; k < K; ++k) cu[k] = total[k];
    cu[K] = frames, cu[K + 1] = entries;
    int32_t* st = stats + g * 4;
    st[0] = ctk_focal_clamp(frames), st[1] = index, st[2] = ctk_focal_clamp(entries), st[3] = bits;
  }
  return 0;
}

#ifdef FOCAL_HOST_MAIN
#include <stdio.h>

// A planted camera path that turns, over G groups, R ring rows and N points; positions, labels, matrices and candidates are spoiled
// here and there (NaN, infinities, positions far outside, a zero matrix, a NaN matrix, candidates that do not stand); every source form
// is run once, the second call of each on the curve of the first.  What a sanitizer build of this file runs (g++ -O1 -g
// -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -DFOCAL_HOST_MAIN).
int main() {
  uint32_t lcg = 12345u;
  auto rnd = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (double)(lcg >> 8) / 16777216.0;
  };
  const float fl = 432.0f, cx = 240.0f, cy = 135.0f;
  uint64_t sum = 0;
  int fitted = 0, rows = 0;
  for (int N : {8, 40, 257, 4200}) {
    for (int K : {1, 3, 64, 256}) {
      if (N == 4200 && K > 3) continue;
      const int G = 2, R = 6, F = 3, f0 = 7, lag = 3, N_out = N > 8 ? N - 1 : N;
      std::vector<float> hc((size_t)G * R * N * 2), anchor((size_t)G * N * 2), fu((size_t)G * F * 9), focals(K);
      std::vector<uint8_t> vis((size_t)G * R * N), av((size_t)G * N);
      std::vector<int8_t> lab((size_t)G * F * N_out), mask((size_t)G * N);
      std::vector<int32_t> first((size_t)G * N, 0);
      for (int k = 0; k < K; ++k) focals[k] = K == 1 ? fl : 120.0f * (float)ldexp(1.0, k * 4 / K) * (1.0f + 0.25f * (float)(k * 4 % K) / (float)K);
      if (K >= 3) focals[1] = N % 2 ? NAN : -5.0f;
      for (int g = 0; g < G; ++g)
        for (int n = 0; n < N; ++n) {
          const double z = 3.0 + 9.0 * rnd(), x = (rnd() - 0.5) * z, y = (rnd() - 0.5) * 0.6 * z;
          mask[(size_t)g * N + n] = n % 13 == 4 ? 0 : (int8_t)(n % 5 - 2 ? n % 5 - 2 : 1);
          av[(size_t)g * N + n] = n % 17 != 2;
          if (n % 23 == 1) first[(size_t)g * N + n] = 8;
          for (int f = f0 - 3; f < f0 + F; ++f) {
            const double a = 0.01 * (f - 4), ca = 1.0 - 0.5 * a * a, sa = a, tx = 0.05 * (f - 4), tz = 0.01 * (f - 4);
            const double X = ca * x + sa * z + tx, Z = -sa * x + ca * z + tz;  // a turn about the vertical axis
            float* c = &hc[(((size_t)g * R + f % R) * N + n) * 2];
            c[0] = (float)(fl * X / Z + cx + 0.1 * (rnd() - 0.5)), c[1] = (float)(fl * y / Z + cy + 0.1 * (rnd() - 0.5));
            if (n % 37 == 9) c[0] = n % 2 ? NAN : 1e9f;
            vis[((size_t)g * R + f % R) * N + n] = rnd() < 0.95;
            if (f == f0 - 3) anchor[((size_t)g * N + n) * 2] = c[0], anchor[((size_t)g * N + n) * 2 + 1] = c[1];
          }
        }
      for (size_t i = 0; i < lab.size(); ++i) lab[i] = (int8_t)(i % 7 == 0 ? 0 : (i % 31 == 0 ? -1 : 1));
      // matrices of a sideways camera that turns a little (not fitted: the rules must cope with whatever they are given)
      for (int i = 0; i < G * F; ++i) {
        float* m = &fu[(size_t)i * 9];
        const float e[9] = {0.0f, -0.02f, 0.01f, 0.02f + 0.001f * i, 0.0f, -1.0f, -0.012f, 1.0f, 0.0f};
        for (int j = 0; j < 9; ++j) {
          const int r = j / 3, c = j % 3;
          const float kr = r < 2 ? 1.0f / fl : 1.0f, kc = c < 2 ? 1.0f / fl : 1.0f;
          m[j] = e[j] * kr * kc;
        }
        // K^-T E K^-1 with the principal point folded in: the third row and column
        m[2] = -(m[0] * cx + m[1] * cy) + e[2] / fl, m[5] = -(m[3] * cx + m[4] * cy) + e[5] / fl;
        m[6] = -(m[0] * cx + m[3] * cy) + e[6] / fl, m[7] = -(m[1] * cx + m[4] * cy) + e[7] / fl;
        m[8] = -(m[6] * cx + m[7] * cy) - (e[2] * cx + e[5] * cy) / fl;
        if (i == 1) for (int j = 0; j < 9; ++j) m[j] = 0.0f;
        if (i == 4) m[4] = NAN;
      }
      std::vector<float> focal(G);
      std::vector<int64_t> curve((size_t)G * (K + 2)), curve2((size_t)G * (K + 2)), cost((size_t)G * F * K);
      std::vector<int32_t> stats((size_t)G * 4);
      for (int form = 0; form < 4; ++form) {
        const bool anchored = form == 2, logits = form == 3;
        std::vector<float> hv, hf;
        if (logits) {
          hv.resize(vis.size()), hf.assign(vis.size(), 6.0f);
          for (size_t i = 0; i < vis.size(); ++i) hv[i] = vis[i] ? 5.0f : -5.0f;
        }
        for (int call = 0; call < 2; ++call) {
          const int rc = host_fit_focal(G, N, N_out, R, f0, F, form == 1 ? 5 : -1, form == 0 || form == 3 ? lag : 0, anchored ? 4 : 0,
                                        N > 8 ? 8 + form : 8, K, 1 + call, cx, cy, 1.0f, 1.0f, 0.6f, 1.0f + form, call ? 1.0f : 1.5f,
                                        hc.data(), logits ? nullptr : vis.data(), logits ? hv.data() : nullptr, logits ? hf.data() : nullptr,
                                        form % 2 ? first.data() : nullptr, anchored ? anchor.data() : nullptr, anchored ? av.data() : nullptr,
                                        form ? mask.data() : nullptr, fu.data(), lab.data(), focals.data(), call ? curve.data() : nullptr,
                                        focal.data(), call ? curve2.data() : curve.data(), cost.data(), stats.data());
          if (rc != 0) return 2;
          for (int g = 0; g < G; ++g) {
            ++rows, fitted += stats[(size_t)g * 4 + 1] >= 0;
            uint32_t b;
            __builtin_memcpy(&b, &focal[g], 4);
            sum = sum * 31u + b + (uint64_t)stats[(size_t)g * 4 + 2];
          }
          for (int64_t v : call ? curve2 : curve) sum = sum * 31u + (uint64_t)v;
          for (int64_t v : cost) sum = sum * 31u + (uint64_t)v;
        }
      }
    }
  }
  printf("%d rows fitted of %d, checksum %016llx\n", fitted, rows, (unsigned long long)sum);
  return fitted > 0 ? 0 : 3;
}
#endif
