// A dense displacement field from the tracked points, and pictures carried along it (include/ctk.h, "track field"), by the rules stated
// once in field_math.h.  No atomics anywhere; every output element is one plain store.
//
// track_field  three launches.
//   accum      gather, not scatter: one workgroup of 256 threads per (group, frame, 16 x 16 node tile), a thread owns one node and keeps
//              its three int64 sums in registers.  The slots are walked in chunks of 256, one slot per thread: the thread quantises
//              the pair once, and the pairs that can reach the tile (inside its box grown by rad) take their place in a 4 KiB LDS list
//              by a wave ballot and a prefix count (wave totals through LDS); then every thread walks the list (all lanes read one
//              LDS address: a broadcast) and adds what reaches its node.  Integer sums: the order does not matter.  The tile at the
//              origin also counts M.  Level 0 of the pyramid goes to the workspace.
//   pyramid    one workgroup of 1024 threads per (group, frame) sums level l into level l + 1, a barrier between two levels (a level
//              is written and read by this workgroup only), and counts the nodes of level 0 that have support and the highest level
//              a node will be filled from: level l is used iff a node of level l has support and a child of it has none.
//   resolve    one thread per node walks up from level 0 to the first level with support, divides once per component and writes the
//              value and the level.
// warp_field   one launch, warp.hip's shape: grid z is the picture, a workgroup owns a tile of 64 x 16 output pixels and one thread makes 4
//              consecutive pixels of one row for all channels.  The field's nodes round the tile (at most 17 x 5) go to LDS first;
//              a pixel's displacement is a convex combination of the four nodes of its cell, rounded, so the minimum and maximum over
//              the tile's nodes bound the tile's source box.  The box -- clamped into the picture, so every clamped tap index lies in
//              it -- is staged in 16 KiB of LDS with whole-dword loads where a box row allows (a box row keeps its address phase, so
//              the dwords go in aligned; nothing outside the box is read); a box that does not fit is sampled from memory with byte
//              loads.  dst goes out as whole dwords when dst, its row stride and its frame stride are multiples of 4 bytes, as
//              bytes otherwise; the W % 4 pixels at the end of a row always go bytewise.  flow goes out as float2.  All frame and
//              row offsets are 64-bit.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "field_math.h"
#include "fit_device.h"  // fit_scale_ok

namespace {

constexpr int FIELD_CHUNK = 256, FIELD_TILE = 16, FIELD_PYR_THREADS = 1024;

struct FieldParams {
  int G, N, N_out, R, f0, F, cs, radius, to, lag, anchor_frame, gh, gw;
  float sx, sy, thresh;
  const float* hc;
  const uint8_t* visible;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
  const float* ac;
  const uint8_t* av;
  int64_t* pyr;
  int64_t nodes;  // of all levels of one (group, frame)
  int32_t* field;
  uint8_t* level;
  int32_t* stats;
};

// grid: x = node tile (row-major over ceil(gw / 16) x ceil(gh / 16)), y = frame f0 + y, z = group
__global__ __launch_bounds__(256) void field_accum_kernel(FieldParams p) {
  __shared__ int4 pts[FIELD_CHUNK];  // (Px, Py, d.x, d.y)
  __shared__ int wave_keep[4], wave_hits[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int pic = (int)blockIdx.y, f = p.f0 + pic;
  const long g = (long)blockIdx.z;
  const int tw = (p.gw + FIELD_TILE - 1) / FIELD_TILE;
  const int ti = (int)blockIdx.x % tw, tj = (int)blockIdx.x / tw;
  const int i = ti * FIELD_TILE + (tid & (FIELD_TILE - 1)), j = tj * FIELD_TILE + tid / FIELD_TILE;
  const int sh = p.cs + 4, rad = p.radius << sh;
  const int Nx = i << sh, Ny = j << sh;
  // a pair reaches a node of the tile iff it lies strictly inside this box on both axes
  const int x_lo = ((ti * FIELD_TILE) << sh) - rad, x_hi = ((ti * FIELD_TILE + FIELD_TILE - 1) << sh) + rad;
  const int y_lo = ((tj * FIELD_TILE) << sh) - rad, y_hi = ((tj * FIELD_TILE + FIELD_TILE - 1) << sh) + rad;
  const bool anchored = p.ac != nullptr;
  const int ft = ctk_field_to(f, p.to, p.lag, anchored, p.anchor_frame);
  const long row_p = (g * p.R + f % p.R) * p.N;
  const long row_q = anchored ? g * p.N : (ft >= 0 ? (g * p.R + ft % p.R) * p.N : 0);
  const float* qc = anchored ? p.ac : p.hc;

  int64_t s[3] = {0, 0, 0};
  int M = 0;
  for (int c0 = 0; c0 < p.N_out; c0 += FIELD_CHUNK) {
    const int n = c0 + tid;
    bool hit = false;
    int4 pt = make_int4(0, 0, 0, 0);
    if (n < p.N_out && ft >= 0) {
      const int first = p.first_row != nullptr ? p.first_row[g * p.N + n] : 0;
      if (f >= first && ft >= first) {
        const float2 hp = *reinterpret_cast<const float2*>(p.hc + (row_p + n) * 2);
        const float2 hq = *reinterpret_cast<const float2*>(qc + (row_q + n) * 2);
        if (ctk_field_pair(hp.x, hp.y, hq.x, hq.y, p.sx, p.sy, &pt.x, &pt.y, &pt.z, &pt.w)) {
          const bool vp = p.visible != nullptr ? p.visible[row_p + n] != 0 : ctk_draw_visible(p.hv[row_p + n], p.hf[row_p + n], p.thresh);
          bool vq;
          if (anchored) vq = p.av[row_q + n] != 0;
          else if (p.visible != nullptr) vq = p.visible[row_q + n] != 0;
          else vq = ctk_draw_visible(p.hv[row_q + n], p.hf[row_q + n], p.thresh);
          hit = vp && vq;
        }
      }
    }
    const bool keep = hit && pt.x > x_lo && pt.x < x_hi && pt.y > y_lo && pt.y < y_hi;
    const unsigned long long mask = __ballot(keep);
    const int hits = __popcll(__ballot(hit));
    if (lane == 0) wave_keep[wave] = __popcll(mask), wave_hits[wave] = hits;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int k = wave_keep[w];
      before += w < wave ? k : 0;
      total += k;
      M += wave_hits[w];
    }
    if (keep) pts[before + __popcll(mask & below)] = pt;
    __syncthreads();
    for (int m = 0; m < total; ++m) {
      const int4 q = pts[m];
      const int w = ctk_field_weight(q.x, q.y, Nx, Ny, p.cs, p.radius);
      if (w != 0) ctk_field_accumulate(s, w, q.z, q.w);
    }
    __syncthreads();  // the list and the wave totals are written again only behind it
  }
  if (i < p.gw && j < p.gh) {
    int64_t* e = p.pyr + ((g * p.F + pic) * p.nodes + (int64_t)j * p.gw + i) * 3;
    e[0] = s[0], e[1] = s[1], e[2] = s[2];
  }
  if (blockIdx.x == 0 && tid == 0) p.stats[(g * p.F + pic) * 4] = M;
}

// grid: x = frame, y = group
__global__ __launch_bounds__(FIELD_PYR_THREADS) void field_pyramid_kernel(FieldParams p) {
  __shared__ int wave_used[FIELD_PYR_THREADS / 64], wave_count[FIELD_PYR_THREADS / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long gf = (long)blockIdx.y * p.F + blockIdx.x;
  int64_t* base = p.pyr + gf * p.nodes * 3;
  int used = 0, count0 = 0, h = p.gh, w = p.gw, l = 0;
  int64_t off = 0;
  while (!(h == 1 && w == 1)) {
    const int h2 = (h + 1) >> 1, w2 = (w + 1) >> 1;
    const int64_t off2 = off + (int64_t)h * w;
    for (int idx = tid; idx < h2 * w2; idx += FIELD_PYR_THREADS) {
      const int J = idx / w2, I = idx - J * w2;
      int64_t s0 = 0, s1 = 0, s2 = 0;
      bool empty_child = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int cj = 2 * J + (k >> 1), ci = 2 * I + (k & 1);
        if (cj < h && ci < w) {
          const int64_t* e = base + (off + (int64_t)cj * w + ci) * 3;
          const int64_t wn = e[0];
          s0 += wn, s1 += e[1], s2 += e[2];
          empty_child = empty_child || wn < 1;
          count0 += l == 0 && wn >= 1 ? 1 : 0;
        }
      }
      int64_t* o = base + (off2 + idx) * 3;
      o[0] = s0, o[1] = s1, o[2] = s2;
      if (s0 >= 1 && empty_child) used = l + 1;  // (l only grows)
    }
    __syncthreads();  // level l + 1 is complete, and visible to this workgroup, before it is read
    off = off2, h = h2, w = w2, ++l;
  }
  const bool any = base[off * 3] >= 1;  // the 1 x 1 level
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(used, o, 64);
    used = u > used ? u : used;
    count0 += __shfl_xor(count0, o, 64);
  }
  if (lane == 0) wave_used[wave] = used, wave_count[wave] = count0;
  __syncthreads();
  if (tid == 0) {
    used = 0, count0 = 0;
    for (int k = 0; k < FIELD_PYR_THREADS / 64; ++k) used = wave_used[k] > used ? wave_used[k] : used, count0 += wave_count[k];
    int32_t* st = p.stats + gf * 4;
    st[1] = count0, st[2] = any ? used : CTK_FIELD_NO_LEVEL, st[3] = 0;
  }
}

// grid: x = ceil(gh * gw / 256), y = frame, z = group
__global__ __launch_bounds__(256) void field_resolve_kernel(FieldParams p) {
  const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (idx >= p.gh * p.gw) return;
  const long gf = (long)blockIdx.z * p.F + blockIdx.y;
  const int j = idx / p.gw, i = idx - j * p.gw;
  int fx, fy;
  const int l = ctk_field_resolve(p.pyr + gf * p.nodes * 3, p.gh, p.gw, j, i, &fx, &fy);
  const long o = gf * ((long)p.gh * p.gw) + idx;
  *reinterpret_cast<int2*>(p.field + o * 2) = make_int2(fx, fy);
  p.level[o] = (uint8_t)l;
}

// everything but the pointers
int field_check_shape(const ctk_track_field_args* a) {
  const long big = 1L << 30;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->R <= 0 || a->F <= 0 || a->N_out > a->N || a->N_out > CTK_FIELD_POINTS_MAX) return CTK_E_SHAPE;
  if (a->f0 < 0 || (long)a->f0 + a->F > big || a->F > 65535 || a->G > 65535 || (long)a->G * a->N > (1L << 26) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->H < 1 || a->H > CTK_INGEST_MAX_SIDE || a->W < 1 || a->W > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->cs < CTK_FIELD_CS_MIN || a->cs > CTK_FIELD_CS_MAX || a->radius < 1 || a->radius > CTK_FIELD_RADIUS_MAX) return CTK_E_SHAPE;
  const bool anchored = a->anchor_coords != nullptr || a->anchor_visible != nullptr;
  if (a->to < -1 || a->to > big || a->lag > big || a->lag < -big) return CTK_E_SHAPE;
  if ((a->to >= 0 ? 1 : 0) + (a->lag != 0 ? 1 : 0) + (anchored ? 1 : 0) != 1) return CTK_E_SHAPE;
  if (anchored) {
    if (a->anchor_frame < 0 || a->anchor_frame > big || a->F > a->R) return CTK_E_SHAPE;
  } else if (a->lag != 0) {
    if ((long)a->F + (a->lag < 0 ? -(long)a->lag : (long)a->lag) > a->R) return CTK_E_SHAPE;
  } else {
    const long lo = a->to < a->f0 ? a->to : a->f0, hi = a->to > (long)a->f0 + a->F - 1 ? a->to : (long)a->f0 + a->F - 1;
    if (hi - lo + 1 > a->R) return CTK_E_SHAPE;
  }
  if (!fit_scale_ok(a->sx) || !fit_scale_ok(a->sy)) return CTK_E_SHAPE;
  if (a->visible == nullptr && a->thresh != a->thresh) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_track_field_workspace_bytes(const ctk_track_field_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = field_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = (size_t)a->G * a->F * (size_t)ctk_field_nodes(ctk_field_grid(a->H, a->cs), ctk_field_grid(a->W, a->cs)) * 24u;
  return CTK_OK;
}

extern "C" int ctk_track_field(const ctk_track_field_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->hist_coords || !a->field || !a->level || !a->stats || !workspace) return CTK_E_NULL;
  if (!a->visible && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  if ((a->anchor_coords != nullptr) != (a->anchor_visible != nullptr)) return CTK_E_NULL;
  const int rc = field_check_shape(a);
  if (rc != CTK_OK) return rc;
  size_t need = 0;
  ctk_track_field_workspace_bytes(a, &need);
  if (workspace_bytes < need) return CTK_E_SHAPE;
  if (((reinterpret_cast<uintptr_t>(a->hist_coords) | reinterpret_cast<uintptr_t>(a->anchor_coords) | reinterpret_cast<uintptr_t>(a->field) |
        reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
    return CTK_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(a->stats) & 3u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  FieldParams p;
  p.G = a->G, p.N = a->N, p.N_out = a->N_out, p.R = a->R, p.f0 = a->f0, p.F = a->F, p.cs = a->cs, p.radius = a->radius;
  p.to = a->to, p.lag = a->lag, p.anchor_frame = a->anchor_frame;
  p.gh = ctk_field_grid(a->H, a->cs), p.gw = ctk_field_grid(a->W, a->cs);
  p.sx = a->sx, p.sy = a->sy, p.thresh = a->thresh;
  p.hc = a->hist_coords, p.visible = a->visible, p.hv = a->hist_vis, p.hf = a->hist_conf, p.first_row = a->first_row;
  p.ac = a->anchor_coords, p.av = a->anchor_visible;
  p.pyr = static_cast<int64_t*>(workspace), p.nodes = ctk_field_nodes(p.gh, p.gw);
  p.field = a->field, p.level = a->level, p.stats = a->stats;
  const double gf = (double)a->G * a->F, grid = (double)p.gh * p.gw;
  const unsigned tiles = (unsigned)(((p.gw + FIELD_TILE - 1) / FIELD_TILE) * ((p.gh + FIELD_TILE - 1) / FIELD_TILE));
  {
    CtkProfScope prof("field_accum", 0.0, gf * (tiles * (double)a->N_out * 18.0 + grid * 24.0), s);
    hipLaunchKernelGGL(field_accum_kernel, dim3(tiles, (unsigned)a->F, (unsigned)a->G), dim3(256), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  {
    CtkProfScope prof("field_pyramid", 0.0, gf * (double)p.nodes * 48.0, s);
    hipLaunchKernelGGL(field_pyramid_kernel, dim3((unsigned)a->F, (unsigned)a->G), dim3(FIELD_PYR_THREADS), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  {
    CtkProfScope prof("field_resolve", 0.0, gf * grid * 33.0, s);
    hipLaunchKernelGGL(field_resolve_kernel, dim3((unsigned)((p.gh * p.gw + 255) / 256), (unsigned)a->F, (unsigned)a->G), dim3(256), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

// ---- warp_field -----------------------------------------------------------------------------------------------------------------------
namespace {

struct WarpFieldParams {
  int H, W, cs, gh, gw, border;
  long src_frame, src_row, dst_frame, dst_row;
  uint32_t fill;  // fill[0] | fill[1] << 8 | fill[2] << 16
  bool dwords;
  const int32_t* field;
  const uint8_t* src;
  uint8_t* dst;
  float* flow;
};

constexpr int WF_PX = 4, WF_TILE_W = 64, WF_TILE_H = 16, WF_LDS_BYTES = 16384;
constexpr int WF_NODES_W = WF_TILE_W / 4 + 1, WF_NODES_H = WF_TILE_H / 4 + 1;  // at the smallest cell: 17 x 5

// Element (ch, y, x) of a picture: channels-last (PLANAR false; C = 1 is this one) or planar.
template <int C, bool PLANAR>
struct WfDirect {
  const uint8_t* frame;
  long row;
  int H;
  __device__ __forceinline__ int operator()(int ch, int y, int x) const {
    return PLANAR ? frame[((long)ch * H + y) * row + x] : frame[(long)y * row + (long)x * C + ch];
  }
};

template <int C, bool PLANAR>
struct WfStaged {
  const uint8_t* lds;
  int bx0, by0, bh, pitch;
  unsigned base_lo, row_lo;  // (address of box row 0) & 3, row stride & 3
  int H;
  __device__ __forceinline__ int operator()(int ch, int y, int x) const {
    const int r = PLANAR ? ch * bh + (y - by0) : y - by0;
    const unsigned g = PLANAR ? (unsigned)(ch * H + (y - by0)) : (unsigned)(y - by0);  // rows from box row 0 in memory
    const unsigned ph = (base_lo + g * row_lo) & 3u;
    return lds[r * pitch + (int)ph + (PLANAR ? x - bx0 : (x - bx0) * C + ch)];
  }
};

// The 4 output pixels (ox .. ox + 3, oy) of picture `pic`; nodes: the tile's nodes in LDS, nw across, the first one (ni0, nj0).
template <int C, bool PLANAR, bool SAMPLE, typename Fetch>
__device__ __forceinline__ void wf_pixels(const WarpFieldParams& p, int pic, int ox, int oy, const int2* nodes, int nw, int ni0, int nj0,
                                          const Fetch& fetch) {
  const int n = p.W - ox < WF_PX ? p.W - ox : WF_PX;  // pixels of this thread that exist
  const int c1 = (1 << p.cs) - 1;
  const int jn = (oy >> p.cs) - nj0, ay = oy & c1;
  uint8_t o[C][WF_PX];
  float2 fl[WF_PX];
#pragma unroll
  for (int k = 0; k < WF_PX; ++k) {
    fl[k] = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[ch][k] = 0;
    if (k >= n) continue;
    const int x = ox + k, in = (x >> p.cs) - ni0, ax = x & c1;
    const int2 f00 = nodes[jn * nw + in], f01 = nodes[jn * nw + in + 1], f10 = nodes[(jn + 1) * nw + in], f11 = nodes[(jn + 1) * nw + in + 1];
    const int64_t dx = ctk_field_sample(f00.x, f01.x, f10.x, f11.x, ax, ay, p.cs), dy = ctk_field_sample(f00.y, f01.y, f10.y, f11.y, ax, ay, p.cs);
    fl[k] = make_float2(ctk_field_flow(dx), ctk_field_flow(dy));
    if (!SAMPLE) continue;
    const int64_t X = ctk_field_coord(x, dx), Y = ctk_field_coord(oy, dy);
    const int ix = ctk_field_whole(X), iy = ctk_field_whole(Y), fx = ctk_field_frac(X), fy = ctk_field_frac(Y);
    const int x0 = ctk_warp_clamp(ix, p.W), x1 = ctk_warp_clamp(ix + 1, p.W), y0 = ctk_warp_clamp(iy, p.H), y1 = ctk_warp_clamp(iy + 1, p.H);
    const bool inx0 = x0 == ix, inx1 = x1 == ix + 1, iny0 = y0 == iy, iny1 = y1 == iy + 1;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      int p00 = fetch(ch, y0, x0), p01 = fetch(ch, y0, x1), p10 = fetch(ch, y1, x0), p11 = fetch(ch, y1, x1);
      if (p.border == CTK_WARP_FILL) {
        const int fv = (int)((p.fill >> (8 * ch)) & 255u);
        p00 = inx0 && iny0 ? p00 : fv, p01 = inx1 && iny0 ? p01 : fv, p10 = inx0 && iny1 ? p10 : fv, p11 = inx1 && iny1 ? p11 : fv;
      }
      o[ch][k] = (uint8_t)ctk_warp_blend(fx, fy, p00, p01, p10, p11);
    }
  }
  if (p.flow != nullptr) {
    float2* q = reinterpret_cast<float2*>(p.flow) + ((long)pic * p.H + oy) * p.W + ox;
#pragma unroll
    for (int k = 0; k < WF_PX; ++k)
      if (k < n) q[k] = fl[k];
  }
  if (!SAMPLE) return;
  const long xs = PLANAR ? 1 : C;
  uint8_t* out = p.dst + (long)pic * p.dst_frame + (long)oy * p.dst_row + (long)ox * xs;
  const long dplane = PLANAR ? (long)p.H * p.dst_row : 1;
  if (p.dwords && n == WF_PX) {
    if (C == 3 && !PLANAR) {
      uint32_t* q = reinterpret_cast<uint32_t*>(out);
      q[0] = (uint32_t)o[0][0] | (uint32_t)o[1 % C][0] << 8 | (uint32_t)o[2 % C][0] << 16 | (uint32_t)o[0][1] << 24;
      q[1] = (uint32_t)o[1 % C][1] | (uint32_t)o[2 % C][1] << 8 | (uint32_t)o[0][2] << 16 | (uint32_t)o[1 % C][2] << 24;
      q[2] = (uint32_t)o[2 % C][2] | (uint32_t)o[0][3] << 8 | (uint32_t)o[1 % C][3] << 16 | (uint32_t)o[2 % C][3] << 24;
    } else {
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        *reinterpret_cast<uint32_t*>(out + (long)ch * dplane) =
            (uint32_t)o[ch][0] | (uint32_t)o[ch][1] << 8 | (uint32_t)o[ch][2] << 16 | (uint32_t)o[ch][3] << 24;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < WF_PX; ++k) {
    if (k < n) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) out[(long)ch * dplane + (long)k * xs] = o[ch][k];
    }
  }
}

__device__ __forceinline__ int wf_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// grid: x = ceil(W / 64), y = ceil(H / 16), z = picture.  SAMPLE false: flow only, nothing of src or dst is touched.
template <int C, bool PLANAR, bool SAMPLE>
__global__ __launch_bounds__(256) void warp_field_kernel(WarpFieldParams p) {
  __shared__ uint32_t lds[SAMPLE ? WF_LDS_BYTES / 4 : 1];
  __shared__ int2 nodes[WF_NODES_W * WF_NODES_H];
  __shared__ int wave_box[4][4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, pic = (int)blockIdx.z;
  const int tx0 = (int)blockIdx.x * WF_TILE_W, ty0 = (int)blockIdx.y * WF_TILE_H;
  const int tx1 = min(tx0 + WF_TILE_W, p.W) - 1, ty1 = min(ty0 + WF_TILE_H, p.H) - 1;  // the tile's last pixel
  // the nodes round the tile: those of the cells its pixels lie in
  const int ni0 = tx0 >> p.cs, nj0 = ty0 >> p.cs;
  const int nw = (tx1 >> p.cs) + 2 - ni0, nh = (ty1 >> p.cs) + 2 - nj0;  // <= 17, <= 5; ni0 + nw - 1 <= gw - 1
  // minus the minimum and the maximum of both components: four maxima
  int bx[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
  if (tid < nw * nh) {
    const int nj = tid / nw, ni = tid - nj * nw;
    const int2 v = *reinterpret_cast<const int2*>(p.field + (((long)pic * p.gh + nj0 + nj) * p.gw + ni0 + ni) * 2);
    nodes[tid] = v;
    // (a field handed in may hold INT32_MIN, whose negative does not exist: one short, and either way far beyond the clamp below)
    bx[0] = v.x == INT32_MIN ? INT32_MAX : -v.x, bx[1] = v.x, bx[2] = v.y == INT32_MIN ? INT32_MAX : -v.y, bx[3] = v.y;
  }
  if (SAMPLE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int m = wf_wave_max(bx[k]);
      if (lane == 0) wave_box[wave][k] = m;
    }
  }
  __syncthreads();
  const int oy = ty0 + tid / (WF_TILE_W / WF_PX), ox = tx0 + (tid % (WF_TILE_W / WF_PX)) * WF_PX;
  const bool mine = oy < p.H && ox < p.W;
  if (!SAMPLE) {
    const WfDirect<C, PLANAR> none = {nullptr, 0, 0};
    if (mine) wf_pixels<C, PLANAR, false>(p, pic, ox, oy, nodes, nw, ni0, nj0, none);
    return;
  }
  int mx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) mx[k] = max(max(wave_box[0][k], wave_box[1][k]), max(wave_box[2][k], wave_box[3][k]));
  // displacements in [-mx[0], mx[1]] x [-mx[2], mx[3]] (1/256 pixel): the whole parts of the tile's coordinates
  const int64_t xa = (int64_t)tx0 * 256 - mx[0], xb = (int64_t)tx1 * 256 + mx[1], ya = (int64_t)ty0 * 256 - mx[2], yb = (int64_t)ty1 * 256 + mx[3];
  const int bx0 = ctk_warp_clamp(ctk_field_whole(xa), p.W), bx1 = ctk_warp_clamp(ctk_field_whole(xb) + 1, p.W);
  const int by0 = ctk_warp_clamp(ctk_field_whole(ya), p.H), by1 = ctk_warp_clamp(ctk_field_whole(yb) + 1, p.H);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const int row_bytes = PLANAR ? bw : bw * C, rows = PLANAR ? bh * C : bh;
  const int pitch = (row_bytes + 6) & ~3;  // a phase of up to 3 bytes in front, rounded up to dwords
  const bool staged = (long)rows * pitch <= WF_LDS_BYTES;
  const uint8_t* frame = p.src + (long)pic * p.src_frame;
  if (!staged) {
    const WfDirect<C, PLANAR> fetch = {frame, p.src_row, p.H};
    if (mine) wf_pixels<C, PLANAR, true>(p, pic, ox, oy, nodes, nw, ni0, nj0, fetch);
    return;
  }
  const uint8_t* box = frame + (long)by0 * p.src_row + (long)bx0 * (PLANAR ? 1 : C);  // box row 0 (of plane 0)
  const int nd = pitch / 4;
  for (int idx = tid; idx < rows * nd; idx += 256) {
    const int r = idx / nd, d = idx - r * nd;
    const long g = PLANAR ? (long)(r / bh) * p.H + (r % bh) : r;  // memory rows from box row 0
    const uint8_t* b0 = box + g * p.src_row;                      // the first and one past the last byte of the box row
    const uint8_t* b1 = b0 + row_bytes;
    const uint8_t* q = b0 - (reinterpret_cast<uintptr_t>(b0) & 3u) + 4 * d;  // an aligned dword of memory
    uint32_t v = 0;
    if (q >= b0 && q + 4 <= b1) {
      v = *reinterpret_cast<const uint32_t*>(q);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q + k >= b0 && q + k < b1) v |= (uint32_t)q[k] << (8 * k);
    }
    lds[r * nd + d] = v;
  }
  __syncthreads();
  const WfStaged<C, PLANAR> fetch = {reinterpret_cast<const uint8_t*>(lds), bx0, by0, bh, pitch,
                                     (unsigned)(reinterpret_cast<uintptr_t>(box) & 3u), (unsigned)(p.src_row & 3), p.H};
  if (mine) wf_pixels<C, PLANAR, true>(p, pic, ox, oy, nodes, nw, ni0, nj0, fetch);
}

template <int C, bool PLANAR>
void warp_field_launch(const WarpFieldParams& p, int F, hipStream_t s) {
  const dim3 grid((unsigned)((p.W + WF_TILE_W - 1) / WF_TILE_W), (unsigned)((p.H + WF_TILE_H - 1) / WF_TILE_H), (unsigned)F);
  if (p.dst != nullptr) hipLaunchKernelGGL((warp_field_kernel<C, PLANAR, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((warp_field_kernel<C, PLANAR, false>), grid, dim3(256), 0, s, p);
}

// elements from the first to one past the last byte of F pictures; rows: pixel rows of a picture, row_elems: elements of one
int64_t wf_extent(int F, int64_t rows, int64_t row_elems, int64_t frame_stride, int64_t row_stride) {
  return (int64_t)(F - 1) * frame_stride + (rows - 1) * row_stride + row_elems;
}

}  // namespace

extern "C" int ctk_warp_field(const ctk_warp_field_args* a, void* stream) {
  if (!a || !a->field || (!a->dst && !a->flow) || (a->dst && !a->src)) return CTK_E_NULL;
  if (a->F < 1 || a->F > 65535 || a->H < 1 || a->H > CTK_INGEST_MAX_SIDE || a->W < 1 || a->W > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->C != 1 && a->C != 3) return CTK_E_SHAPE;
  if (a->layout != CTK_INGEST_HWC && a->layout != CTK_INGEST_CHW) return CTK_E_SHAPE;
  if (a->border != CTK_WARP_FILL && a->border != CTK_WARP_EDGE) return CTK_E_SHAPE;
  if (a->cs < CTK_FIELD_CS_MIN || a->cs > CTK_FIELD_CS_MAX || a->reserved != 0) return CTK_E_SHAPE;
  const bool planar = a->layout == CTK_INGEST_CHW && a->C == 3;
  const int64_t rows = planar ? (int64_t)a->H * a->C : a->H, row_elems = planar ? a->W : (int64_t)a->W * a->C;
  bool dwords = false;
  if (a->dst) {
    const int64_t big = (int64_t)1 << 40;
    const int64_t strides[2][2] = {{a->src_frame_stride, a->src_row_stride}, {a->dst_frame_stride, a->dst_row_stride}};
    for (int k = 0; k < 2; ++k) {
      const int64_t frame = strides[k][0], row = strides[k][1];
      if (row < row_elems || row > big || frame > big) return CTK_E_SHAPE;
      if (frame < row * rows && !(k == 0 && frame == 0)) return CTK_E_SHAPE;  // (src_frame_stride 0: one source for every picture)
    }
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(a->src), d0 = reinterpret_cast<uintptr_t>(a->dst);
    const uintptr_t s1 = s0 + (uintptr_t)wf_extent(a->F, rows, row_elems, a->src_frame_stride, a->src_row_stride);
    const uintptr_t d1 = d0 + (uintptr_t)wf_extent(a->F, rows, row_elems, a->dst_frame_stride, a->dst_row_stride);
    if (s0 < d1 && d0 < s1) return CTK_E_SHAPE;  // a warp cannot run in place
    // whole dwords: every 4-pixel group of every row of every picture (and plane) then starts on a 4-byte multiple of the base
    dwords = (d0 & 3u) == 0 && a->dst_row_stride % 4 == 0 && (a->F == 1 || a->dst_frame_stride % 4 == 0);
  }
  if ((reinterpret_cast<uintptr_t>(a->field) & 7u) != 0 || (reinterpret_cast<uintptr_t>(a->flow) & 7u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  WarpFieldParams p;
  p.H = a->H, p.W = a->W, p.cs = a->cs, p.gh = ctk_field_grid(a->H, a->cs), p.gw = ctk_field_grid(a->W, a->cs), p.border = a->border;
  p.src_frame = (long)a->src_frame_stride, p.src_row = (long)a->src_row_stride;
  p.dst_frame = (long)a->dst_frame_stride, p.dst_row = (long)a->dst_row_stride;
  p.fill = (uint32_t)a->fill[0] | (uint32_t)a->fill[1] << 8 | (uint32_t)a->fill[2] << 16;
  p.dwords = dwords;
  p.field = a->field, p.src = a->src, p.dst = a->dst, p.flow = a->flow;
  {
    const double px = (double)a->F * a->H * a->W;
    CtkProfScope prof("warp_field", 0.0, px * ((a->dst ? 2.0 * a->C : 0.0) + (a->flow ? 8.0 : 0.0)), s);
    if (a->C == 1) warp_field_launch<1, false>(p, a->F, s);
    else if (planar) warp_field_launch<3, true>(p, a->F, s);
    else warp_field_launch<3, false>(p, a->F, s);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
