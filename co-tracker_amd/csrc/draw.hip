// Tracks drawn onto uint8 frames on the device (include/ctk.h, "draw tracks"): marks and fading trails of every point, by the
// integer rules stated once in draw_math.h.  Two launches, no atomics, no fill.
//
// 1. prepare: one thread per primitive slot of every picture.  The slots of a picture are in DRAW ORDER -- segments k = L .. 1, then
//    the marks, each g-then-n -- and a slot's index is its place in that order: no compaction, so the table does not depend on
//    scheduling.  The thread reads the history (and takes the expf of the logits) once and writes a fixed-size record of 24 bytes,
//    kept as two planes so that the scan below reads only what it tests:
//      bounds  2 dwords: x0 | x1 << 16, y0 | y1 << 16 -- the inclusive pixel bounding box clipped to the picture; an absent
//              primitive (or one wholly outside) has the box x0 = y0 = 65535, x1 = y1 = 0, which meets no tile (x0 lies beyond
//              every tile: sides are <= 32768)
//      body    4 dwords: colour | alpha << 24;  ax;  ay;  (dx + 4096) | (dy + 4096) << 13 | kind << 26 | visible << 27 | present << 28
//              (A = the mark's centre or the segment's first end, d = B - A; kind 1 = segment)
// 2. raster: one workgroup of 256 threads per tile of 128 x 8 pixels per picture, a thread owning 4 consecutive pixels of one row.
//    The workgroup scans its picture's table in chunks of 256 records, one record per thread: the threads whose record's box meets
//    the tile take their place in an LDS list by a wave ballot and a prefix count (wave totals through LDS), which keeps the
//    table's order; the list is then applied to the pixels in registers, every thread reading the same LDS record (a broadcast),
//    chunk after chunk.  In place, pixels are loaded when the first record meets the tile and a thread stores only what it
//    changed: a tile that nothing meets is neither read nor written.  With src != dst every pixel is copied.
//    Channels-last rows move as dwords -- 4 pixels are 12 bytes, three dwords per thread, 384 contiguous bytes per 32 lanes --
//    when base and strides are multiples of 4 bytes (planar: one dword per plane); the last, partial group of a row and
//    unaligned surfaces go byte by byte.  No byte beyond W pixels of a row is read or written.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "draw_math.h"

namespace {

constexpr int DRAW_TW = 128, DRAW_TH = 8, DRAW_PX = 4;  // tile; pixels per thread
constexpr int DRAW_CHUNK = 256;
constexpr unsigned DRAW_EMPTY_BX = 0xffffu, DRAW_EMPTY_BY = 0xffffu;  // x0 = y0 = 65535 > every tile's last pixel; x1 = y1 = 0

struct DrawPrep {
  int G, N, N_out, R, f0, L, radius, hw, max_jump, H, W;
  float sx, sy, thresh;
  const float* hc;
  const uint8_t* visible;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
  const uint8_t* colors;
  uint8_t alpha[CTK_DRAW_TRAIL_MAX + 1];
};

struct DrawPoint {
  bool shown, visible;
  int qx, qy;
};

// frame fr of slot (g, n): shown, visible and the pixel.  Nothing is read for a frame below 0 or below the slot's first row.
__device__ __forceinline__ DrawPoint draw_point(const DrawPrep& p, long g, int n, int fr, int first) {
  DrawPoint o;
  o.shown = false, o.visible = false, o.qx = 0, o.qy = 0;
  if (fr < 0 || fr < first) return o;
  const long row = (g * p.R + fr % p.R) * p.N + n;
  const float2 h = *reinterpret_cast<const float2*>(p.hc + row * 2);
  const bool okx = ctk_draw_quant(h.x, p.sx, &o.qx), oky = ctk_draw_quant(h.y, p.sy, &o.qy);
  o.shown = okx && oky;
  if (!o.shown) return o;
  o.visible = p.visible != nullptr ? p.visible[row] != 0 : ctk_draw_visible(p.hv[row], p.hf[row], p.thresh);
  return o;
}

// grid: x = ceil(P / 256), y = picture; P = (L + 1) * G * N_out slots per picture
__global__ __launch_bounds__(256) void draw_prepare_kernel(DrawPrep p, long P, uint2* __restrict__ bounds, uint4* __restrict__ body) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= P) return;
  const long per = (long)p.G * p.N_out;
  const int k = p.L - (int)(s / per);  // L .. 1: segments; 0: marks
  const long rem = s % per;
  const long g = rem / p.N_out;
  const int n = (int)(rem % p.N_out);
  const int f = p.f0 + (int)blockIdx.y;
  const int first = p.first_row != nullptr ? p.first_row[g * p.N + n] : 0;
  bool present = false, visible = false;
  int ax = 0, ay = 0, dx = 0, dy = 0, x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  if (k == 0) {
    const DrawPoint c = draw_point(p, g, n, f, first);
    if (c.shown) {
      present = true, visible = c.visible, ax = c.qx, ay = c.qy;
      x0 = ax - p.radius, x1 = ax + p.radius, y0 = ay - p.radius, y1 = ay + p.radius;
    }
  } else {
    const DrawPoint a = draw_point(p, g, n, f - k, first);
    if (a.shown && a.visible) {
      const DrawPoint b = draw_point(p, g, n, f - k + 1, first);
      if (b.shown && b.visible) {
        dx = b.qx - a.qx, dy = b.qy - a.qy;  // (|q| <= 65536: no overflow)
        if (dx >= -p.max_jump && dx <= p.max_jump && dy >= -p.max_jump && dy <= p.max_jump) {
          present = true, visible = true, ax = a.qx, ay = a.qy;
          x0 = min(ax, b.qx) - p.hw, x1 = max(ax, b.qx) + p.hw, y0 = min(ay, b.qy) - p.hw, y1 = max(ay, b.qy) + p.hw;
        } else {
          dx = 0, dy = 0;
        }
      }
    }
  }
  uint2 bb = make_uint2(DRAW_EMPTY_BX, DRAW_EMPTY_BY);
  if (present) {
    x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, p.W - 1), y1 = min(y1, p.H - 1);  // (sides <= 32768: 15 bits each)
    if (x0 <= x1 && y0 <= y1) bb = make_uint2((unsigned)x0 | (unsigned)x1 << 16, (unsigned)y0 | (unsigned)y1 << 16);
  }
  const uint8_t* c = p.colors + (g * p.N + n) * 3;
  uint4 r;
  r.x = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 | (unsigned)p.alpha[k] << 24;
  r.y = (unsigned)ax, r.z = (unsigned)ay;
  r.w = (unsigned)(dx + 4096) | (unsigned)(dy + 4096) << 13 | (k != 0 ? 1u << 26 : 0u) | (visible ? 1u << 27 : 0u) | (present ? 1u << 28 : 0u);
  const long at = (long)blockIdx.y * P + s;
  bounds[at] = bb;
  body[at] = r;
}

struct DrawRaster {
  const uint8_t* src;
  uint8_t* dst;
  long frame_stride, row_stride;
  int H, W, radius, hw, tiles_x;
  bool in_place;
};

// the 4 pixels of a thread: px[i][c]; x + i < W only for i < n
template <int LAYOUT, bool VEC>
__device__ __forceinline__ void draw_load(const uint8_t* __restrict__ q, long plane, int n, int (&px)[DRAW_PX][3]) {
  if (LAYOUT == CTK_INGEST_HWC) {
    if (VEC && n == DRAW_PX) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(q);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      const uint32_t b[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255,
                              (w1 >> 16) & 255, w1 >> 24, w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
#pragma unroll
      for (int i = 0; i < DRAW_PX; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) px[i][c] = (int)b[i * 3 + c];
    } else {
#pragma unroll
      for (int i = 0; i < DRAW_PX; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) px[i][c] = i < n ? (int)q[i * 3 + c] : 0;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* qc = q + (long)c * plane;
      if (VEC && n == DRAW_PX) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(qc);
#pragma unroll
        for (int i = 0; i < DRAW_PX; ++i) px[i][c] = (int)((w >> (8 * i)) & 255);
      } else {
#pragma unroll
        for (int i = 0; i < DRAW_PX; ++i) px[i][c] = i < n ? (int)qc[i] : 0;
      }
    }
  }
}

template <int LAYOUT, bool VEC>
__device__ __forceinline__ void draw_store(uint8_t* __restrict__ q, long plane, int n, const int (&px)[DRAW_PX][3]) {
  if (LAYOUT == CTK_INGEST_HWC) {
    if (VEC && n == DRAW_PX) {
      uint32_t w[3] = {0, 0, 0};
#pragma unroll
      for (int i = 0; i < DRAW_PX; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) w[(i * 3 + c) >> 2] |= (uint32_t)px[i][c] << (8 * ((i * 3 + c) & 3));
      uint32_t* o = reinterpret_cast<uint32_t*>(q);
      o[0] = w[0], o[1] = w[1], o[2] = w[2];
    } else {
#pragma unroll
      for (int i = 0; i < DRAW_PX; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (i < n) q[i * 3 + c] = (uint8_t)px[i][c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint8_t* qc = q + (long)c * plane;
      if (VEC && n == DRAW_PX) {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < DRAW_PX; ++i) w |= (uint32_t)px[i][c] << (8 * i);
        *reinterpret_cast<uint32_t*>(qc) = w;
      } else {
#pragma unroll
        for (int i = 0; i < DRAW_PX; ++i)
          if (i < n) qc[i] = (uint8_t)px[i][c];
      }
    }
  }
}

// grid: x = tiles_x * tiles_y, y = picture
template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(256) void draw_raster_kernel(DrawRaster p, long P, const uint2* __restrict__ bounds, const uint4* __restrict__ body) {
  __shared__ uint4 list[DRAW_CHUNK];
  __shared__ int wave_hits[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_y = (int)blockIdx.x / p.tiles_x, tile_x = (int)blockIdx.x - tile_y * p.tiles_x;
  const int tx0 = tile_x * DRAW_TW, ty0 = tile_y * DRAW_TH;
  const int tx1 = min(tx0 + DRAW_TW, p.W) - 1, ty1 = min(ty0 + DRAW_TH, p.H) - 1;
  const int x = tx0 + (tid & 31) * DRAW_PX, y = ty0 + (tid >> 5);
  const int n = y < p.H ? min(max(p.W - x, 0), DRAW_PX) : 0;  // this thread's pixels inside the picture
  const long plane = (long)p.H * p.row_stride;
  const long off = (long)blockIdx.y * p.frame_stride + (long)y * p.row_stride + (LAYOUT == CTK_INGEST_HWC ? (long)x * 3 : (long)x);
  int px[DRAW_PX][3];
#pragma unroll
  for (int i = 0; i < DRAW_PX; ++i) px[i][0] = px[i][1] = px[i][2] = 0;
  bool loaded = false, dirty = false;  // (loaded is block-uniform)
  if (!p.in_place) {
    if (n > 0) draw_load<LAYOUT, VEC>(p.src + off, plane, n, px);
    loaded = true;
  }
  const uint2* tb = bounds + (long)blockIdx.y * P;
  const uint4* tr = body + (long)blockIdx.y * P;
  for (long c0 = 0; c0 < P; c0 += DRAW_CHUNK) {
    const long s = c0 + tid;
    bool hit = false;
    if (s < P) {
      const uint2 bb = tb[s];
      const int x0 = (int)(bb.x & 0xffff), x1 = (int)(bb.x >> 16), y0 = (int)(bb.y & 0xffff), y1 = (int)(bb.y >> 16);
      hit = x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wave_hits[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int h = wave_hits[w];
      before += w < wave ? h : 0;
      total += h;
    }
    if (hit) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = tr[s];
    if (total > 0 && !loaded) {  // in place: the first record that meets the tile
      if (n > 0) draw_load<LAYOUT, VEC>(p.dst + off, plane, n, px);
      loaded = true;
    }
    __syncthreads();
    if (n > 0) {
      for (int j = 0; j < total; ++j) {
        const uint4 r = list[j];
        const int ax = (int)r.y, ay = (int)r.z;
        const int dx = (int)(r.w & 0x1fff) - 4096, dy = (int)((r.w >> 13) & 0x1fff) - 4096;
        const bool seg = (r.w >> 26) & 1u, vis = (r.w >> 27) & 1u;
        const int a = (int)(r.x >> 24);
        const int cr = (int)(r.x & 255), cg = (int)((r.x >> 8) & 255), cb = (int)((r.x >> 16) & 255);
#pragma unroll
        for (int i = 0; i < DRAW_PX; ++i) {
          const int ox = x + i - ax, oy = y - ay;
          const bool cov = seg ? ctk_draw_segment_covers(ox, oy, dx, dy, p.hw) : ctk_draw_mark_covers(ox, oy, p.radius, vis);
          if (cov && i < n) {
            px[i][0] = ctk_draw_blend(px[i][0], cr, a);
            px[i][1] = ctk_draw_blend(px[i][1], cg, a);
            px[i][2] = ctk_draw_blend(px[i][2], cb, a);
            dirty = true;
          }
        }
      }
    }
    // No third barrier: the next chunk writes wave_hits after the second barrier above, behind which nobody reads it any more, and
    // writes the list after its own first barrier, which a thread reaches only when it has applied this chunk's list.
  }
  if (n > 0 && (dirty || !p.in_place)) draw_store<LAYOUT, VEC>(p.dst + off, plane, n, px);
}

template <int LAYOUT>
void draw_raster_launch(const DrawRaster& p, long P, int F, const uint2* bounds, const uint4* body, bool vec, hipStream_t s) {
  const int tiles_y = (p.H + DRAW_TH - 1) / DRAW_TH;
  const dim3 grid((unsigned)(p.tiles_x * tiles_y), (unsigned)F);
  if (vec) hipLaunchKernelGGL((draw_raster_kernel<LAYOUT, true>), grid, dim3(256), 0, s, p, P, bounds, body);
  else hipLaunchKernelGGL((draw_raster_kernel<LAYOUT, false>), grid, dim3(256), 0, s, p, P, bounds, body);
}

// everything but the pointers; *P = the slots of one picture
int draw_check_shape(const ctk_draw_args* a, long* P) {
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->R <= 0 || a->F <= 0 || a->N_out > a->N) return CTK_E_SHAPE;
  if (a->trail < 0 || a->trail > CTK_DRAW_TRAIL_MAX || a->radius < 1 || a->radius > CTK_DRAW_RADIUS_MAX) return CTK_E_SHAPE;
  if (a->half_width < 0 || a->half_width > CTK_DRAW_HALF_WIDTH_MAX || a->max_jump < 1 || a->max_jump > CTK_DRAW_JUMP_MAX) return CTK_E_SHAPE;
  if (a->f0 < 0 || (long)a->f0 + a->F > (1L << 30) || (long)a->F + a->trail > a->R || a->F > 65535) return CTK_E_SHAPE;
  if (a->G > 65535 || (long)a->G * a->N > (1L << 26) || a->reserved != 0) return CTK_E_SHAPE;
  if (a->layout != CTK_INGEST_HWC && a->layout != CTK_INGEST_CHW) return CTK_E_SHAPE;
  if (a->H < 1 || a->W < 1 || a->H > CTK_INGEST_MAX_SIDE || a->W > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  const bool hwc = a->layout == CTK_INGEST_HWC;
  if (a->row_stride < (int64_t)a->W * (hwc ? 3 : 1)) return CTK_E_SHAPE;
  if (a->row_stride > (int64_t)1 << 40 || a->frame_stride > (int64_t)1 << 40) return CTK_E_SHAPE;
  if (a->frame_stride < a->row_stride * a->H * (hwc ? 1 : 3)) return CTK_E_SHAPE;
  if (a->visible == nullptr && a->thresh != a->thresh) return CTK_E_SHAPE;
  *P = (long)(a->trail + 1) * a->G * a->N_out;  // <= 65 * 2^26: a grid of at most 2^25 blocks of 256
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_draw_tracks_workspace_bytes(const ctk_draw_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  long P = 0;
  const int rc = draw_check_shape(a, &P);
  if (rc != CTK_OK) return rc;
  *out_bytes = (size_t)P * (size_t)a->F * (sizeof(uint2) + sizeof(uint4));
  return CTK_OK;
}

extern "C" int ctk_draw_tracks(const ctk_draw_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->hist_coords || !a->colors || !a->dst || !workspace) return CTK_E_NULL;
  if (!a->visible && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  long P = 0;
  const int rc = draw_check_shape(a, &P);
  if (rc != CTK_OK) return rc;
  const size_t slots = (size_t)P * (size_t)a->F;
  if (workspace_bytes < slots * (sizeof(uint2) + sizeof(uint4))) return CTK_E_SHAPE;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || (reinterpret_cast<uintptr_t>(a->hist_coords) & 7u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint4* body = static_cast<uint4*>(workspace);  // the 16-byte plane first: both planes keep their alignment
  uint2* bounds = reinterpret_cast<uint2*>(body + slots);

  DrawPrep pp;
  pp.G = a->G, pp.N = a->N, pp.N_out = a->N_out, pp.R = a->R, pp.f0 = a->f0, pp.L = a->trail;
  pp.radius = a->radius, pp.hw = a->half_width, pp.max_jump = a->max_jump, pp.H = a->H, pp.W = a->W;
  pp.sx = a->sx, pp.sy = a->sy, pp.thresh = a->thresh;
  pp.hc = a->hist_coords, pp.visible = a->visible, pp.hv = a->hist_vis, pp.hf = a->hist_conf;
  pp.first_row = a->first_row, pp.colors = a->colors;
  for (int k = 0; k <= CTK_DRAW_TRAIL_MAX; ++k) pp.alpha[k] = a->alpha[k];
  {
    CtkProfScope prof("draw_prepare", 0.0, (double)slots * 24.0, s);
    hipLaunchKernelGGL(draw_prepare_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)a->F), dim3(256), 0, s, pp, P, bounds, body);
  }
  CTK_HIP_CHECK_LAUNCH();

  DrawRaster rp;
  rp.dst = a->dst, rp.src = a->src ? a->src : a->dst, rp.in_place = a->src == nullptr || a->src == a->dst;
  rp.frame_stride = (long)a->frame_stride, rp.row_stride = (long)a->row_stride;
  rp.H = a->H, rp.W = a->W, rp.radius = a->radius, rp.hw = a->half_width, rp.tiles_x = (a->W + DRAW_TW - 1) / DRAW_TW;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(rp.dst) | reinterpret_cast<uintptr_t>(rp.src) | (uintptr_t)a->frame_stride |
                         (uintptr_t)a->row_stride;
  const bool vec = (bits & 3u) == 0;  // every 4-pixel group of every row and plane then starts on a dword
  {
    CtkProfScope prof("draw_raster", 0.0, (double)a->F * a->H * a->W * 3.0 * (rp.in_place ? 1.0 : 2.0), s);
    if (a->layout == CTK_INGEST_HWC) draw_raster_launch<CTK_INGEST_HWC>(rp, P, a->F, bounds, body, vec, s);
    else draw_raster_launch<CTK_INGEST_CHW>(rp, P, a->F, bounds, body, vec, s);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
