// Host build of co-tracker_amd/csrc/field_math.h behind plain loops, as a stand-alone program: the rules of ctk_track_field and
// ctk_warp_field (include/ctk.h, "track field") without a GPU (tests/test_field_host.py; also built there with
// -fsanitize=address,undefined).  Compile with -ffp-contract=off, like the device unit.
//   field_host track IN OUT   IN: int32 head[16] = G N N_out R f0 F H W cs radius to lag anchor_frame has_visible has_first_row has_anchor,
//                             float32 sx sy thresh, coords [G,R,N,2], then visible uint8 [G,R,N] or vis, conf float32 [G,R,N], then
//                             first_row int32 [G,N] and anchor coords float32 [G,N,2], visible uint8 [G,N] where announced
//                             OUT: field int32 [G,F,gh,gw,2], level uint8 [G,F,gh,gw], stats int32 [G,F,4]
//   field_host warp IN OUT    IN: int32 head[12] = F H W C layout border cs fill0 fill1 fill2 src_pictures(1 or F) 0, field int32
//                             [F,gh,gw,2], src uint8 (dense); OUT: dst uint8 (dense), flow float32 [F,H,W,2]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../co-tracker_amd/csrc/field_math.h"

namespace {

template <typename T>
std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n != 0 && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "field_host: short input\n");
    exit(2);
  }
  return v;
}

template <typename T>
void put(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
}

int track(FILE* in, FILE* out) {
  const std::vector<int32_t> h = take<int32_t>(in, 16);
  const int G = h[0], N = h[1], N_out = h[2], R = h[3], f0 = h[4], F = h[5], H = h[6], W = h[7], cs = h[8], radius = h[9], to = h[10], lag = h[11];
  const int anchor_frame = h[12];
  const bool has_visible = h[13] != 0, has_first = h[14] != 0, anchored = h[15] != 0;
  const std::vector<float> sc = take<float>(in, 3);
  const size_t rows = (size_t)G * R * N;
  const std::vector<float> hc = take<float>(in, rows * 2);
  const std::vector<uint8_t> visible = take<uint8_t>(in, has_visible ? rows : 0);
  const std::vector<float> hv = take<float>(in, has_visible ? 0 : rows), hf = take<float>(in, has_visible ? 0 : rows);
  const std::vector<int32_t> first_row = take<int32_t>(in, has_first ? (size_t)G * N : 0);
  const std::vector<float> ac = take<float>(in, anchored ? (size_t)G * N * 2 : 0);
  const std::vector<uint8_t> av = take<uint8_t>(in, anchored ? (size_t)G * N : 0);
  const int gh = ctk_field_grid(H, cs), gw = ctk_field_grid(W, cs), sh = cs + 4;
  const int64_t nodes = ctk_field_nodes(gh, gw);
  std::vector<int32_t> field((size_t)G * F * gh * gw * 2), stats((size_t)G * F * 4);
  std::vector<uint8_t> level((size_t)G * F * gh * gw);
  std::vector<int64_t> pyr((size_t)nodes * 3);
  std::vector<int> P;  // (Px, Py, dx, dy) per pair
  for (int64_t g = 0; g < G; ++g)
    for (int k = 0; k < F; ++k) {
      const int f = f0 + k, ft = ctk_field_to(f, to, lag, anchored, anchor_frame);
      P.clear();
      for (int n = 0; n < N_out && ft >= 0; ++n) {
        const int first = has_first ? first_row[g * N + n] : 0;
        if (!(f >= first && ft >= first)) continue;
        const int64_t rp = (g * R + f % R) * N + n, rq = anchored ? g * N + n : (g * R + ft % R) * N + n;
        const float* q = anchored ? ac.data() : hc.data();
        int v[4];
        if (!ctk_field_pair(hc[rp * 2], hc[rp * 2 + 1], q[rq * 2], q[rq * 2 + 1], sc[0], sc[1], &v[0], &v[1], &v[2], &v[3])) continue;
        const bool vp = has_visible ? visible[rp] != 0 : ctk_draw_visible(hv[rp], hf[rp], sc[2]);
        const bool vq = anchored ? av[rq] != 0 : (has_visible ? visible[rq] != 0 : ctk_draw_visible(hv[rq], hf[rq], sc[2]));
        if (vp && vq) P.insert(P.end(), v, v + 4);
      }
      for (int j = 0; j < gh; ++j)
        for (int i = 0; i < gw; ++i) {
          int64_t s[3] = {0, 0, 0};
          for (size_t m = 0; m < P.size(); m += 4) {
            const int w = ctk_field_weight(P[m], P[m + 1], i << sh, j << sh, cs, radius);
            if (w != 0) ctk_field_accumulate(s, w, P[m + 2], P[m + 3]);
          }
          for (int c = 0; c < 3; ++c) pyr[((size_t)j * gw + i) * 3 + c] = s[c];
        }
      int64_t off = 0;
      for (int hh = gh, ww = gw; !(hh == 1 && ww == 1);) {
        const int h2 = (hh + 1) >> 1, w2 = (ww + 1) >> 1;
        const int64_t off2 = off + (int64_t)hh * ww;
        for (int J = 0; J < h2; ++J)
          for (int I = 0; I < w2; ++I)
            for (int c = 0; c < 3; ++c) {
              int64_t s = 0;
              for (int t = 0; t < 4; ++t) {
                const int cj = 2 * J + (t >> 1), ci = 2 * I + (t & 1);
                if (cj < hh && ci < ww) s += pyr[(off + (int64_t)cj * ww + ci) * 3 + c];
              }
              pyr[(off2 + (int64_t)J * w2 + I) * 3 + c] = s;
            }
        off = off2, hh = h2, ww = w2;
      }
      int at0 = 0, used = 0;
      for (int j = 0; j < gh; ++j)
        for (int i = 0; i < gw; ++i) {
          int fx, fy;
          const int l = ctk_field_resolve(pyr.data(), gh, gw, j, i, &fx, &fy);
          const size_t o = ((size_t)(g * F + k) * gh + j) * gw + i;
          field[o * 2] = fx, field[o * 2 + 1] = fy, level[o] = (uint8_t)l;
          at0 += l == 0 ? 1 : 0, used = l > used ? l : used;
        }
      int32_t* st = &stats[(size_t)(g * F + k) * 4];
      st[0] = (int)(P.size() / 4), st[1] = at0, st[2] = used, st[3] = 0;
    }
  put(out, field), put(out, level), put(out, stats);
  return 0;
}

int warp(FILE* in, FILE* out) {
  const std::vector<int32_t> h = take<int32_t>(in, 12);
  const int F = h[0], H = h[1], W = h[2], C = h[3], layout = h[4], border = h[5], cs = h[6], pictures = h[10];
  const uint8_t fill[3] = {(uint8_t)h[7], (uint8_t)h[8], (uint8_t)h[9]};
  const int gh = ctk_field_grid(H, cs), gw = ctk_field_grid(W, cs), c1 = (1 << cs) - 1;
  const std::vector<int32_t> field = take<int32_t>(in, (size_t)F * gh * gw * 2);
  const size_t pic = (size_t)H * W * C;
  const std::vector<uint8_t> src = take<uint8_t>(in, pic * pictures);
  std::vector<uint8_t> dst(pic * F);
  std::vector<float> flow((size_t)F * H * W * 2);
  const bool planar = layout == 1 && C == 3;
  for (int p = 0; p < F; ++p) {
    const int32_t* fd = &field[(size_t)p * gh * gw * 2];
    const uint8_t* s = &src[pictures == 1 ? 0 : pic * p];
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int i = x >> cs, ax = x & c1, j = y >> cs, ay = y & c1;
        const int32_t *n00 = fd + ((size_t)j * gw + i) * 2, *n01 = n00 + 2, *n10 = n00 + (size_t)gw * 2, *n11 = n10 + 2;
        const int64_t dx = ctk_field_sample(n00[0], n01[0], n10[0], n11[0], ax, ay, cs), dy = ctk_field_sample(n00[1], n01[1], n10[1], n11[1], ax, ay, cs);
        float* fl = &flow[(((size_t)p * H + y) * W + x) * 2];
        fl[0] = ctk_field_flow(dx), fl[1] = ctk_field_flow(dy);
        const int64_t X = ctk_field_coord(x, dx), Y = ctk_field_coord(y, dy);
        const int ix = ctk_field_whole(X), iy = ctk_field_whole(Y), fx = ctk_field_frac(X), fy = ctk_field_frac(Y);
        for (int ch = 0; ch < C; ++ch) {
          int t[4];
          for (int k = 0; k < 4; ++k) {
            const int tx = ix + (k & 1), ty = iy + (k >> 1);
            const bool inside = tx >= 0 && tx < W && ty >= 0 && ty < H;
            const size_t cy = (size_t)ctk_warp_clamp(ty, H), cx = (size_t)ctk_warp_clamp(tx, W);
            if (border == CTK_WARP_FILL && !inside) t[k] = fill[ch];
            else t[k] = planar ? s[((size_t)ch * H + cy) * W + cx] : s[(cy * W + cx) * C + ch];
          }
          const uint8_t v = (uint8_t)ctk_warp_blend(fx, fy, t[0], t[1], t[2], t[3]);
          if (planar) dst[pic * p + ((size_t)ch * H + y) * W + x] = v;
          else dst[pic * p + ((size_t)y * W + x) * C + ch] = v;
        }
      }
  }
  put(out, dst), put(out, flow);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: field_host track|warp IN OUT\n");
    return 1;
  }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 1;
  const int rc = argv[1][0] == 't' ? track(in, out) : warp(in, out);
  fclose(in);
  return fclose(out) != 0 ? 1 : rc;
}
