// Host build of co-tracker_amd/csrc/align_math.h behind plain loops: the rules of ctk_fit_align (include/ctk.h, "fit align") without
// workgroups, LDS or a GPU (tests/test_align_host.py).  Compile with -ffp-contract=off, like the device unit.  With -DALIGN_HOST_MAIN
// the file is a stand-alone program that runs the same function on inputs it makes itself (a planted similarity, spoiled points in
// either set, collinear and repeated triples, identical sets, the list cap) and prints a checksum: what a sanitizer build of it runs.
#include <stdint.h>

#include <vector>

#include "../../co-tracker_amd/csrc/align_math.h"

// three entries (X, Y: nine doubles each) -> 1 and thirteen doubles (s, nine of R, three of t), or 0 and (1, I, 0)
extern "C" int host_align_candidate(const double* X, const double* Y, double* out) {
  CtkAlign c;
  const bool ok = ctk_align_candidate(X, Y, &c);
  out[0] = c.s;
  for (int i = 0; i < 9; ++i) out[1 + i] = c.R[i];
  for (int i = 0; i < 3; ++i) out[10 + i] = c.t[i];
  return ok ? 1 : 0;
}

// The whole of ctk_fit_align, one pair after the other; the arguments are the fields of ctk_fit_align_args.
// -> 0, or -2 where min_points, hypotheses, tol or depth_tol is refused
extern "C" int host_fit_align(int G, int N, int min_points, int hypotheses, uint32_t seed, float fx, float fy, float cx, float cy, float tol,
                              float depth_tol, const float* a, const int8_t* valid_a, const float* b, const int8_t* valid_b,
                              const uint8_t* mask, float* sim, float* scale, int8_t* label, float* error, int32_t* stats) {
  if (min_points < CTK_ALIGN_MIN_POINTS || min_points > CTK_MOTION_POINTS_MAX) return -2;
  if (hypotheses < 1 || hypotheses > CTK_RESECTION_HYPOTHESES_MAX) return -2;
  if (!(tol > 0.0f) || !ctk_resection_finite32(tol) || !(depth_tol > 0.0f) || !ctk_resection_finite32(depth_tol)) return -2;
  const CtkPoseCam cam = {(double)fx, (double)fy, (double)cx, (double)cy};
  const double tol2 = ctk_resection_tol2(tol), dtol = (double)depth_tol;
  const int K = hypotheses;
  const CtkAlignWeights weights = ctk_align_weights(cam, tol, depth_tol);
  struct Pt { int n; double X[3], Y[3]; };
  std::vector<Pt> all, list;
  for (long g = 0; g < G; ++g) {
    int8_t* lab = label + g * N;
    float* err = error + g * N;
    float* so = sim + g * 12L;
    int32_t* st = stats + g * 4L;
    all.clear(), list.clear();
    int same = 0, listed = 0;
    for (int n = 0; n < N; ++n) {
      lab[n] = -1, err[n] = -1.0f;
      Pt t;
      t.n = n;
      bool eq;
      const long o = g * N + n;
      if (!ctk_align_point(a + o * 3, valid_a[o], b + o * 3, valid_b[o], t.X, t.Y, &eq)) continue;
      lab[n] = 0;
      same += eq ? 1 : 0;
      all.push_back(t);
      if (mask == nullptr || mask[o] != 0) {
        if (listed < CTK_RESECTION_LIST_MAX) list.push_back(t);
        ++listed;
      }
    }
    const int M = (int)list.size();
    const bool identical = !all.empty() && same == (int)all.size();
    int bits = (listed > CTK_RESECTION_LIST_MAX ? CTK_RESECTION_BIT_CAP : 0) | (identical ? CTK_RESECTION_BIT_STILL : 0);
    for (int i = 0; i < 12; ++i) so[i] = 0.0f;
    scale[g] = 0.0f;
    st[0] = M, st[1] = 0, st[2] = -1, st[3] = bits;
    if (M < CTK_ALIGN_MIN_POINTS) continue;
    int best = -1, bk = -1;
    CtkAlign cur;
    ctk_align_eye(&cur);
    // (backwards: the winner does not depend on the order the candidates are made and scored in)
    for (int k = K; k >= (identical ? K : 0); --k) {
      CtkAlign c;
      ctk_align_eye(&c);
      if (k < K) {
        int idx[3];
        double X[9], Y[9];
        ctk_align_sample(seed, k, M, idx);
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) X[i * 3 + j] = list[idx[i]].X[j], Y[i * 3 + j] = list[idx[i]].Y[j];
        if (!ctk_align_candidate(X, Y, &c)) continue;
      }
      int cnt = 0;
      for (int m = 0; m < M; ++m) {
        double Z[3];
        ctk_align_apply(c, list[m].X, Z);
        cnt += ctk_align_within(cam, Z, list[m].Y, tol2, dtol) ? 1 : 0;
      }
      if (bk < 0 || ctk_resection_better(cnt, k, best, bk)) best = cnt, bk = k, cur = c;
    }
    if (best < min_points) continue;
    for (int round = 0; round < CTK_ALIGN_ROUNDS; ++round) {
      const double gate2 = ctk_structure_gate2(tol, round), dgate = ctk_align_dgate(depth_tol, round);
      int reach = CTK_ALIGN_NO_REACH;
      for (int m = 0; m < M; ++m) {
        double Z[3];
        ctk_align_apply(cur, list[m].X, Z);
        if (!ctk_align_within(cam, Z, list[m].Y, gate2, dgate)) continue;
        const int e = ctk_align_reach(list[m].Y);
        reach = e > reach ? e : reach;
      }
      int64_t s[CTK_ALIGN_SUMS];
      for (int i = 0; i < CTK_ALIGN_SUMS; ++i) s[i] = 0;
      int n = 0;
      // (backwards: the sums do not depend on the order of accumulation)
      for (int m = M; m-- > 0;) {
        double Z[3], v[24];
        ctk_align_apply(cur, list[m].X, Z);
        if (!ctk_align_within(cam, Z, list[m].Y, gate2, dgate)) continue;
        if (ctk_align_entry(weights, Z, list[m].Y, reach, v)) {
          ctk_align_terms(v + 16, s);
          ctk_align_terms(v + 8, s);
          ctk_align_terms(v, s);
          ++n;
        } else {
          bits |= CTK_ALIGN_BIT_LEFT;
        }
      }
      double work[CTK_POSE_SOLVE_DOUBLES];
      CtkAlign next;
      if (ctk_align_update(cur, s, n, reach, work, &next)) cur = next;
      else bits |= CTK_ALIGN_BIT_ROUND;
    }
    int ones = 0;
    for (const Pt& t : all) {
      double Z[3];
      ctk_align_apply(cur, t.X, Z);
      lab[t.n] = ctk_align_within(cam, Z, t.Y, tol2, dtol) ? 1 : 0;
      err[t.n] = ctk_align_error(cam, Z, t.Y);
      ones += lab[t.n];
    }
    ctk_align_out(cur, so, &scale[g]);
    st[1] = ones, st[2] = bk, st[3] = bits;
  }
  return 0;
}

#ifdef ALIGN_HOST_MAIN
#include <stdio.h>

// Pairs of point sets under a planted similarity; points, validity bytes and the mask are spoiled here and there (NaN, infinities,
// out-of-range values, points behind the camera, a run of collinear points and a run of copies of one point); one pair is identical.
int main() {
  uint32_t lcg = 12345u;
  auto rnd = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (double)(lcg >> 8) / 16777216.0;
  };
  const float fx = 1000.0f, fy = 990.0f, cx = 960.0f, cy = 540.0f;
  uint64_t sum = 0;
  int fitted = 0, rows = 0;
  for (int N : {3, 7, 40, 257, 4200}) {
    const int G = 3;
    std::vector<float> a((size_t)G * N * 3), b((size_t)G * N * 3);
    std::vector<int8_t> va((size_t)G * N), vb((size_t)G * N);
    std::vector<uint8_t> mask((size_t)G * N);
    for (int g = 0; g < G; ++g) {
      const double s = 0.3 + 3.0 * rnd(), c = 0.9, sn = 0.43588989435406733, tx = rnd() - 0.5, ty = rnd() - 0.5, tz = rnd();
      for (int n = 0; n < N; ++n) {
        const double z = 3.0 + 9.0 * rnd(), x = (rnd() - 0.5) * z, y = (rnd() - 0.5) * 0.6 * z;
        float* pa = &a[((size_t)g * N + n) * 3];
        float* pb = &b[((size_t)g * N + n) * 3];
        pa[0] = (float)x, pa[1] = (float)y, pa[2] = (float)z;
        // b = s R a + t with R a turn about the y axis, and a little noise
        pb[0] = (float)(s * (c * x + sn * z) + tx + 1e-3 * (rnd() - 0.5)), pb[1] = (float)(s * y + ty + 1e-3 * (rnd() - 0.5));
        pb[2] = (float)(s * (-sn * x + c * z) + tz + 3.0);
        if (g == 2) pb[0] = pa[0], pb[1] = pa[1], pb[2] = pa[2];  // the identical pair
        if (n % 5 == 4 && g < 2) pb[0] += 0.5f;                   // a point that moved
        va[(size_t)g * N + n] = n % 11 == 3 ? 0 : (int8_t)(1 + n % 100);
        vb[(size_t)g * N + n] = n % 13 == 5 ? 0 : 1;
        mask[(size_t)g * N + n] = n % 7 != 6;
        if (n % 29 == 8) pa[n % 3] = n % 2 ? NAN : INFINITY;
        if (n % 31 == 9) pb[2] = -pb[2];
        if (n % 37 == 10) pb[n % 3] = 3.0e6f;
        if (g == 0 && n >= 20 && n < 26) pa[0] = 0.25f * (n - 20), pa[1] = 0.5f * (n - 20), pa[2] = 4.0f + 0.125f * (n - 20);  // collinear
        if (g == 0 && n >= 30 && n < 34) pb[0] = 1.0f, pb[1] = -1.0f, pb[2] = 5.0f;                                         // one point, four times
      }
    }
    std::vector<float> sim((size_t)G * 12), scale(G), err((size_t)G * N);
    std::vector<int8_t> lab((size_t)G * N);
    std::vector<int32_t> st((size_t)G * 4);
    for (int form = 0; form < 2; ++form) {
      const int rc = host_fit_align(G, N, 3, form == 0 ? 33 : 1024, 9u + form, fx, fy, cx, cy, 2.0f, 0.1f, a.data(), va.data(), b.data(), vb.data(),
                                    form == 0 ? mask.data() : nullptr, sim.data(), scale.data(), lab.data(), err.data(), st.data());
      if (rc != 0) return 2;
      for (size_t i = 0; i < st.size(); ++i) sum = sum * 31u + (uint32_t)st[i];
      for (size_t i = 0; i < lab.size(); ++i) sum = sum * 31u + (uint8_t)lab[i];
      for (size_t i = 0; i < sim.size(); ++i) {
        uint32_t bits;
        __builtin_memcpy(&bits, &sim[i], 4);
        sum = sum * 31u + bits;
      }
      for (int i = 0; i < G; ++i) fitted += st[(size_t)i * 4 + 2] >= 0, ++rows;
    }
  }
  printf("align_host: %d of %d rows fitted, checksum %016llx\n", fitted, rows, (unsigned long long)sum);
  return fitted > 0 ? 0 : 3;
}
#endif
