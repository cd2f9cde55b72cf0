// Host build of co-tracker_amd/csrc/structure_math.h behind plain loops: the rules of ctk_fit_structure (include/ctk.h, "fit structure")
// without workgroups, LDS or a GPU (tests/test_structure_host.py).  Compile with -ffp-contract=off, like the device unit.  With
// -DSTRUCTURE_HOST_MAIN the file is a stand-alone program that runs the same function on inputs it makes itself (a planted camera
// path, spoiled positions, poses and old points) and prints a checksum: what a sanitizer build of it runs.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/structure_math.h"

// twelve floats -> the view counts; out: nine doubles of R, three of t, three of c
extern "C" int host_structure_view(const float* m, int stats_ok, double* out) {
  CtkStructureView v;
  const bool ok = ctk_structure_view(m, stats_ok != 0, &v);
  for (int i = 0; i < 9; ++i) out[i] = v.p.R[i];
  for (int i = 0; i < 3; ++i) out[9 + i] = v.p.t[i], out[12 + i] = v.c[i];
  return ok ? 1 : 0;
}

// The whole of ctk_fit_structure, one (group, slot) after the other; the arguments are the fields of ctk_fit_structure_args.
// -> 0, or -2 where into, min_views, refine, tol or min_sin2 is refused
extern "C" int host_fit_structure(int G, int N, int N_out, int R, int f0, int F, int into, int source_frame, int min_views, int refine,
                                  float fx, float fy, float cx, float cy, float sx, float sy, float thresh, float tol, float min_sin2,
                                  const float* hc, const uint8_t* visible, const float* hv, const float* hf, const int32_t* first_row,
                                  const float* pose, const int32_t* pose_stats, const float* structure_in, const int8_t* valid_in,
                                  const float* origin_in, float* points, int8_t* label, float* error, int32_t* stats, float* origin_out) {
  if (F < 1 || F > CTK_STRUCTURE_VIEWS_MAX || F > R || into < -1 || into >= F || refine < 0 || refine > 1) return -2;
  if (min_views < CTK_STRUCTURE_MIN_VIEWS || min_views > CTK_STRUCTURE_VIEWS_MAX) return -2;
  if (!(tol > 0.0f) || !ctk_resection_finite32(tol) || !(min_sin2 > 0.0f && min_sin2 <= 1.0f)) return -2;
  if ((structure_in != nullptr) != (valid_in != nullptr)) return -2;
  const CtkPoseCam cam = {(double)fx, (double)fy, (double)cx, (double)cy};
  std::vector<CtkStructureView> views((size_t)F);
  std::vector<uint8_t> counts((size_t)F);
  for (long g = 0; g < G; ++g) {
    for (int j = 0; j < F; ++j)
      counts[j] = ctk_structure_view(pose + (g * F + j) * 12L, pose_stats == nullptr || pose_stats[(g * F + j) * 4L + 2] >= 0, &views[j]) ? 1 : 0;
    const bool into_counts = into >= 0 && counts[into] != 0, no_structure = into >= 0 && !into_counts;
    const CtkStructureView* into_view = into_counts ? &views[into] : nullptr;
    if (origin_out != nullptr) ctk_structure_origin(origin_in != nullptr ? origin_in + g * 12L : nullptr, into_view, origin_out + g * 12L);
    for (int n = 0; n < N_out; ++n) {
      const long gn = g * N + n;
      const bool has_first = first_row != nullptr;
      const int first = has_first ? first_row[gn] : 0;
      bool in_old = false, carried = false;
      float old[3] = {0.0f, 0.0f, 0.0f};
      if (structure_in != nullptr) {
        double Xo[3];
        in_old = ctk_structure_old(structure_in + gn * 3L, valid_in[gn], has_first, first, source_frame, Xo);
        carried = in_old && !no_structure && ctk_structure_out(into_view, Xo, old);
      }
      auto obs = [&](int j, int* qx, int* qy) {
        const int f = f0 + j;
        if (f < first) return false;
        const long at = (g * R + f % R) * N + n;
        const bool okx = ctk_motion_quant(hc[at * 2], sx, qx), oky = ctk_motion_quant(hc[at * 2 + 1], sy, qy);
        if (!(okx && oky)) return false;
        return visible != nullptr ? visible[at] != 0 : ctk_draw_visible(hv[at], hf[at], thresh);
      };
      float point[3] = {0.0f, 0.0f, 0.0f}, err = -1.0f;
      int32_t st[4] = {0, 0, -1, 0};
      int lab;
      if (no_structure) {
        int m = 0;
        for (int j = F; j-- > 0;) {  // (backwards: a count does not depend on the order)
          int qx, qy;
          if (counts[j] != 0 && obs(j, &qx, &qy)) ++m;
        }
        st[0] = m, st[3] = CTK_STRUCTURE_BIT_INTO;
        lab = m >= 1 || in_old ? 0 : -1;
      } else if (carried && refine == 0) {
        point[0] = old[0], point[1] = old[1], point[2] = old[2];
        lab = 2;
      } else {
        lab = ctk_structure_slot(cam, views.data(), counts.data(), F, into_counts ? into : -1, tol, min_sin2, min_views,
                                 carried ? old : nullptr, obs, point, &err, st);
      }
      const long o = g * N_out + n;
      for (int i = 0; i < 3; ++i) points[o * 3 + i] = point[i];
      label[o] = (int8_t)lab, error[o] = err;
      for (int i = 0; i < 4; ++i) stats[o * 4 + i] = st[i];
    }
  }
  return 0;
}

#ifdef STRUCTURE_HOST_MAIN
#include <stdio.h>

// A planted camera path over G groups, R ring rows and N points; positions, poses, pose stats, old points and first rows are spoiled
// here and there; every mode (into, carry, refine, origin, logits) is run.
int main() {
  uint32_t lcg = 4321u;
  auto rnd = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (double)(lcg >> 8) / 16777216.0;
  };
  const float fx = 432.0f, fy = 430.0f, cx = 240.0f, cy = 135.0f;
  uint64_t sum = 0;
  long accepted = 0, slots = 0;
  const int shapes[4][2] = {{1, 1}, {65, 2}, {300, 8}, {70, 256}};
  for (const auto& shape : shapes) {
    const int N = shape[0], F = shape[1], G = 2, R = F < 8 ? 8 : F, f0 = R == F ? 0 : 5, N_out = N > 8 ? N - 1 : N;
    std::vector<float> hc((size_t)G * R * N * 2), hv((size_t)G * R * N), hf((size_t)G * R * N, 5.0f), str((size_t)G * N * 3);
    std::vector<float> pose((size_t)G * F * 12), origin((size_t)G * 12);
    std::vector<uint8_t> vis((size_t)G * R * N);
    std::vector<int8_t> valid((size_t)G * N);
    std::vector<int32_t> first((size_t)G * N, 0), pst((size_t)G * F * 4, 0);
    for (int g = 0; g < G; ++g) {
      for (int j = 0; j < F; ++j) {
        float* s = &pose[((size_t)g * F + j) * 12];
        for (int i = 0; i < 12; ++i) s[i] = i % 5 == 0 ? 1.0f : 0.0f;
        s[3] = -(float)(0.05 * j * (R == 256 ? 0.1 : 1.0)), s[11] = -(float)(0.01 * j), s[1] = 0.002f * j, s[4] = -0.002f * j;
        if (F > 2 && j == 1) s[5] = NAN;
        if (F > 3 && j == 2) for (int i = 0; i < 12; ++i) s[i] = 0.0f;
        if (F > 4 && j == 3) pst[((size_t)g * F + j) * 4 + 2] = -1;
      }
      for (int i = 0; i < 12; ++i) origin[(size_t)g * 12 + i] = i % 5 == 0 ? 1.0f : 0.1f * i;
      for (int n = 0; n < N; ++n) {
        const double z = 3.0 + 9.0 * rnd(), x = (rnd() - 0.5) * z, y = (rnd() - 0.5) * 0.6 * z;
        float* s = &str[((size_t)g * N + n) * 3];
        s[0] = (float)x, s[1] = (float)y, s[2] = (float)z;
        valid[(size_t)g * N + n] = n % 3 == 0 ? 0 : (int8_t)(1 + n % 100);
        if (n % 29 == 5) s[n % 3] = n % 2 ? NAN : INFINITY;
        if (n % 23 == 1) first[(size_t)g * N + n] = f0 + 2;
        for (int j = 0; j < F; ++j) {
          const int f = f0 + j;
          const float* s12 = &pose[((size_t)g * F + j) * 12];
          const double xc = x + s12[1] * y + s12[3], yc = s12[4] * x + y, zc = z + s12[11];
          const size_t at = ((size_t)g * R + f % R) * N + n;
          hc[at * 2] = (float)(fx * xc / zc + cx + 0.1 * (rnd() - 0.5)), hc[at * 2 + 1] = (float)(fy * yc / zc + cy + 0.1 * (rnd() - 0.5));
          if (n % 37 == 9 && j % 2) hc[at * 2] = n % 2 ? NAN : 1e9f;
          if (n % 41 == 11 && j == F - 1) hc[at * 2] += 40.0f;  // one grossly wrong view
          vis[at] = rnd() < 0.9;
          hv[at] = vis[at] ? 4.0f : -4.0f;
        }
      }
    }
    std::vector<float> pts((size_t)G * N_out * 3), err((size_t)G * N_out), oo((size_t)G * 12);
    std::vector<int8_t> lab((size_t)G * N_out);
    std::vector<int32_t> st((size_t)G * N_out * 4);
    for (int mode = 0; mode < 6; ++mode) {
      const int into = mode == 0 ? -1 : (mode == 1 ? 0 : (mode == 2 && F > 2 ? 1 : F - 1));
      const bool carry = mode >= 2, logits = mode == 4;
      const int rc = host_fit_structure(G, N, N_out, R, f0, F, into, f0 + 1, mode == 5 && F >= 3 ? 3 : 2, mode == 3 ? 1 : 0, fx, fy, cx, cy, 1.0f,
                                        1.0f, 0.5f, 2.0f, 3.0e-5f, hc.data(), logits ? nullptr : vis.data(), logits ? hv.data() : nullptr,
                                        logits ? hf.data() : nullptr, mode % 2 ? first.data() : nullptr, pose.data(),
                                        mode == 0 ? nullptr : pst.data(), carry ? str.data() : nullptr, carry ? valid.data() : nullptr,
                                        mode % 2 ? origin.data() : nullptr, pts.data(), lab.data(), err.data(), st.data(), oo.data());
      if (rc != 0) return 2;
      for (size_t i = 0; i < st.size(); ++i) sum = sum * 31u + (uint32_t)st[i];
      for (size_t i = 0; i < lab.size(); ++i) sum = sum * 31u + (uint8_t)lab[i], accepted += lab[i] == 1, ++slots;
      for (size_t i = 0; i < pts.size(); ++i) {
        uint32_t b;
        __builtin_memcpy(&b, &pts[i], 4);
        sum = sum * 31u + b;
      }
      for (size_t i = 0; i < oo.size(); ++i) {
        uint32_t b;
        __builtin_memcpy(&b, &oo[i], 4);
        sum = sum * 31u + b;
      }
    }
  }
  printf("structure_host: %ld of %ld slots accepted, checksum %016llx\n", accepted, slots, (unsigned long long)sum);
  return accepted > 0 ? 0 : 3;
}
#endif
