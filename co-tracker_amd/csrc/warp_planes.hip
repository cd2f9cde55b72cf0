// Pictures resampled under 3 x 3 matrices (include/ctk.h, "fit planes / warp planes"), by the rules of plane_math.h on top of
// warp_math.h's taps and blend.  One launch, no atomics; every byte that is written is written by one plain store, and a byte the
// rule does not write is never touched (CTK_WARP_KEEP draws a picture into frames in place).
//
// warp.hip's shape: grid z is the picture, a workgroup owns a tile of 64 x 16 output pixels and one thread makes 4 consecutive pixels
// of one row for all channels.  A pixel's position is the closed form of plane_math.h -- about ten double operations and one
// division --, never stepped.  The workgroup projects the four corners of its tile: with a finite matrix, Z > 0 and a position within
// reach at all four, the tile's positions lie in the box of the corners' positions (a projective map takes a convex tile on which
// Z > 0 to the convex hull of its corners' images), and one pixel more on every side covers the rounding of the per-pixel arithmetic and
// the second tap.  That box, clamped into the source, is staged in 16 KiB of LDS with whole-dword loads where it fits; otherwise
// (a horizon through the tile, a strong perspective) taps are byte loads from memory.  Taps are read at clamped indices -- nothing
// outside the source is read under any border -- and a staged tap is clamped into the box as well.  Under CTK_WARP_KEEP a tile whose
// box misses the source ends before it samples: it could write nothing.  No other tile is culled.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "plane_math.h"

namespace {

struct WarpPlanesParams {
  int H, W, Hs, Ws, border;
  long src_frame, src_row, dst_frame, dst_row;
  uint32_t fill;  // fill[0] | fill[1] << 8 | fill[2] << 16
  bool dwords;
  const float* matrices;
  const uint8_t* src;
  uint8_t* dst;
};

constexpr int WP_PX = 4, WP_TILE_W = 64, WP_TILE_H = 16, WP_LDS_BYTES = 16384;

// Element (ch, y, x) of a source picture: channels-last (PLANAR false; C = 1 is this one) or planar.
template <int C, bool PLANAR>
struct WpDirect {
  const uint8_t* frame;
  long row;
  int Hs;
  __device__ __forceinline__ int operator()(int ch, int y, int x) const {
    return PLANAR ? frame[((long)ch * Hs + y) * row + x] : frame[(long)y * row + (long)x * C + ch];
  }
};

template <int C, bool PLANAR>
struct WpStaged {
  const uint8_t* lds;
  int bx0, by0, bx1, by1, bh, pitch;
  unsigned base_lo, row_lo;  // (address of box row 0) & 3, row stride & 3
  int Hs;
  __device__ __forceinline__ int operator()(int ch, int y, int x) const {
    y = min(max(y, by0), by1), x = min(max(x, bx0), bx1);
    const int r = PLANAR ? ch * bh + (y - by0) : y - by0;
    const unsigned g = PLANAR ? (unsigned)(ch * Hs + (y - by0)) : (unsigned)(y - by0);  // rows from box row 0 in memory
    const unsigned ph = (base_lo + g * row_lo) & 3u;
    return lds[r * pitch + (int)ph + (PLANAR ? x - bx0 : (x - bx0) * C + ch)];
  }
};

// The 4 output pixels (ox .. ox + 3, oy) of picture `pic`; m: the matrix in doubles, finite: all its entries are.
template <int C, bool PLANAR, typename Fetch>
__device__ __forceinline__ void wp_pixels(const WarpPlanesParams& p, int pic, int ox, int oy, const double* m, bool finite, const Fetch& fetch) {
  const int n = p.W - ox < WP_PX ? p.W - ox : WP_PX;  // pixels of this thread that exist
  uint8_t o[C][WP_PX];
  bool wr[WP_PX];
#pragma unroll
  for (int k = 0; k < WP_PX; ++k) {
    wr[k] = false;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[ch][k] = 0;
    if (k >= n) continue;
    int64_t X = 0, Y = 0;
    const bool inside = finite && ctk_plane_coord(m, ox + k, oy, &X, &Y);
    if (!inside) {
      wr[k] = p.border != CTK_WARP_KEEP;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) o[ch][k] = (uint8_t)((p.fill >> (8 * ch)) & 255u);
      continue;
    }
    const int ix = ctk_plane_whole(X), iy = ctk_plane_whole(Y), fx = ctk_plane_frac(X), fy = ctk_plane_frac(Y);
    const int x0 = ctk_warp_clamp(ix, p.Ws), x1 = ctk_warp_clamp(ix + 1, p.Ws), y0 = ctk_warp_clamp(iy, p.Hs), y1 = ctk_warp_clamp(iy + 1, p.Hs);
    const bool inx0 = x0 == ix, inx1 = x1 == ix + 1, iny0 = y0 == iy, iny1 = y1 == iy + 1;
    wr[k] = p.border != CTK_WARP_KEEP || (inx0 && inx1 && iny0 && iny1);
    if (!wr[k]) continue;
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
  const long xs = PLANAR ? 1 : C;
  uint8_t* out = p.dst + (long)pic * p.dst_frame + (long)oy * p.dst_row + (long)ox * xs;
  const long dplane = PLANAR ? (long)p.H * p.dst_row : 1;
  if (p.dwords && n == WP_PX && wr[0] && wr[1] && wr[2] && wr[3]) {
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
  for (int k = 0; k < WP_PX; ++k) {
    if (k < n && wr[k]) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) out[(long)ch * dplane + (long)k * xs] = o[ch][k];
    }
  }
}

// grid: x = ceil(W / 64), y = ceil(H / 16), z = picture
template <int C, bool PLANAR>
__global__ __launch_bounds__(256) void warp_planes_kernel(WarpPlanesParams p) {
  __shared__ uint32_t lds[WP_LDS_BYTES / 4];
  const int tid = (int)threadIdx.x, pic = (int)blockIdx.z;
  const int tx0 = (int)blockIdx.x * WP_TILE_W, ty0 = (int)blockIdx.y * WP_TILE_H;
  const int tx1 = min(tx0 + WP_TILE_W, p.W) - 1, ty1 = min(ty0 + WP_TILE_H, p.H) - 1;  // the tile's last pixel
  float mf[9];
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) mf[i] = p.matrices[(long)pic * 9 + i];
  const bool finite = ctk_plane_matrix(mf, m);
  const int oy = ty0 + tid / (WP_TILE_W / WP_PX), ox = tx0 + (tid % (WP_TILE_W / WP_PX)) * WP_PX;
  const bool mine = oy < p.H && ox < p.W;
  const uint8_t* frame = p.src + (long)pic * p.src_frame;
  // the box of the four corners' positions, when all four are inside
  bool bounded = finite;
  double lox = CTK_PLANE_REACH, hix = -CTK_PLANE_REACH, loy = CTK_PLANE_REACH, hiy = -CTK_PLANE_REACH;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double v[3], sx = 0.0, sy = 0.0;
    ctk_plane_project(m, k & 1 ? tx1 : tx0, k & 2 ? ty1 : ty0, v);
    bounded = bounded && ctk_plane_position(v, &sx, &sy);
    lox = fmin(lox, sx), hix = fmax(hix, sx), loy = fmin(loy, sy), hiy = fmax(hiy, sy);
  }
  int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0, pitch = 0, rows = 0, row_bytes = 0, bh = 0;
  bool staged = false;
  if (bounded) {  // (|positions| <= 2^20: the conversions cannot overflow)
    const int ux0 = (int)floor(lox) - 1, ux1 = (int)floor(hix) + 2, uy0 = (int)floor(loy) - 1, uy1 = (int)floor(hiy) + 2;
    // Every tap index of the tile lies in [ux0, ux1] x [uy0, uy1].  CTK_WARP_KEEP writes a pixel only when all four of its taps are
    // inside the source: a tile whose box misses the source writes nothing and ends here (uniform over the workgroup).  This is the
    // only culling; it looks at the box, never at whether the tile's corners fall into the picture.
    if (p.border == CTK_WARP_KEEP && (ux1 < 0 || ux0 > p.Ws - 1 || uy1 < 0 || uy0 > p.Hs - 1)) return;
    bx0 = ctk_warp_clamp(ux0, p.Ws), bx1 = ctk_warp_clamp(ux1, p.Ws);
    by0 = ctk_warp_clamp(uy0, p.Hs), by1 = ctk_warp_clamp(uy1, p.Hs);
    const int bw = bx1 - bx0 + 1;
    bh = by1 - by0 + 1;
    row_bytes = PLANAR ? bw : bw * C, rows = PLANAR ? bh * C : bh;
    pitch = (row_bytes + 6) & ~3;  // a phase of up to 3 bytes in front, rounded up to dwords
    staged = (long)rows * pitch <= WP_LDS_BYTES;
  }
  if (!staged) {  // (uniform over the workgroup: the corners are the tile's)
    const WpDirect<C, PLANAR> fetch = {frame, p.src_row, p.Hs};
    if (mine) wp_pixels<C, PLANAR>(p, pic, ox, oy, m, finite, fetch);
    return;
  }
  const uint8_t* box = frame + (long)by0 * p.src_row + (long)bx0 * (PLANAR ? 1 : C);  // box row 0 (of plane 0)
  const int nd = pitch / 4;
  for (int idx = tid; idx < rows * nd; idx += 256) {
    const int r = idx / nd, d = idx - r * nd;
    const long g = PLANAR ? (long)(r / bh) * p.Hs + (r % bh) : r;  // memory rows from box row 0
    const uint8_t* b0 = box + g * p.src_row;                       // the first and one past the last byte of the box row
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
  const WpStaged<C, PLANAR> fetch = {reinterpret_cast<const uint8_t*>(lds), bx0, by0, bx1, by1, bh, pitch,
                                     (unsigned)(reinterpret_cast<uintptr_t>(box) & 3u), (unsigned)(p.src_row & 3), p.Hs};
  if (mine) wp_pixels<C, PLANAR>(p, pic, ox, oy, m, finite, fetch);
}

template <int C, bool PLANAR>
void warp_planes_launch(const WarpPlanesParams& p, int F, hipStream_t s) {
  const dim3 grid((unsigned)((p.W + WP_TILE_W - 1) / WP_TILE_W), (unsigned)((p.H + WP_TILE_H - 1) / WP_TILE_H), (unsigned)F);
  hipLaunchKernelGGL((warp_planes_kernel<C, PLANAR>), grid, dim3(256), 0, s, p);
}

// elements from the first to one past the last byte of F pictures; rows: pixel rows of a picture, row_elems: elements of one
int64_t wp_extent(int F, int64_t rows, int64_t row_elems, int64_t frame_stride, int64_t row_stride) {
  return (int64_t)(F - 1) * frame_stride + (rows - 1) * row_stride + row_elems;
}

}  // namespace

extern "C" int ctk_warp_planes(const ctk_warp_planes_args* a, void* stream) {
  if (!a || !a->matrices || !a->src || !a->dst) return CTK_E_NULL;
  if (a->F < 1 || a->F > 65535 || a->H < 1 || a->H > CTK_INGEST_MAX_SIDE || a->W < 1 || a->W > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->Hs < 1 || a->Hs > CTK_INGEST_MAX_SIDE || a->Ws < 1 || a->Ws > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->C != 1 && a->C != 3) return CTK_E_SHAPE;
  if (a->layout != CTK_INGEST_HWC && a->layout != CTK_INGEST_CHW) return CTK_E_SHAPE;
  if (a->border != CTK_WARP_FILL && a->border != CTK_WARP_EDGE && a->border != CTK_WARP_KEEP) return CTK_E_SHAPE;
  if (a->reserved != 0) return CTK_E_SHAPE;
  const bool planar = a->layout == CTK_INGEST_CHW && a->C == 3;
  const int64_t big = (int64_t)1 << 40;
  const int64_t sizes[2][2] = {{a->Hs, a->Ws}, {a->H, a->W}};
  const int64_t strides[2][2] = {{a->src_frame_stride, a->src_row_stride}, {a->dst_frame_stride, a->dst_row_stride}};
  int64_t ext[2];
  for (int k = 0; k < 2; ++k) {
    const int64_t rows = planar ? sizes[k][0] * a->C : sizes[k][0], row_elems = planar ? sizes[k][1] : sizes[k][1] * a->C;
    const int64_t frame = strides[k][0], row = strides[k][1];
    if (row < row_elems || row > big || frame > big) return CTK_E_SHAPE;
    if (frame < row * rows && !(k == 0 && frame == 0)) return CTK_E_SHAPE;  // (src_frame_stride 0: one source for every picture)
    ext[k] = wp_extent(a->F, rows, row_elems, frame, row);
  }
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(a->src), d0 = reinterpret_cast<uintptr_t>(a->dst);
  const uintptr_t s1 = s0 + (uintptr_t)ext[0], d1 = d0 + (uintptr_t)ext[1];
  if (s0 < d1 && d0 < s1) return CTK_E_SHAPE;  // the source and the destination never overlap
  if ((reinterpret_cast<uintptr_t>(a->matrices) & 3u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  WarpPlanesParams p;
  p.H = a->H, p.W = a->W, p.Hs = a->Hs, p.Ws = a->Ws, p.border = a->border;
  p.src_frame = (long)a->src_frame_stride, p.src_row = (long)a->src_row_stride;
  p.dst_frame = (long)a->dst_frame_stride, p.dst_row = (long)a->dst_row_stride;
  p.fill = (uint32_t)a->fill[0] | (uint32_t)a->fill[1] << 8 | (uint32_t)a->fill[2] << 16;
  // whole dwords: every 4-pixel group of every row of every picture (and plane) then starts on a 4-byte multiple of the base
  p.dwords = (d0 & 3u) == 0 && a->dst_row_stride % 4 == 0 && (a->F == 1 || a->dst_frame_stride % 4 == 0);
  p.matrices = a->matrices, p.src = a->src, p.dst = a->dst;
  {
    CtkProfScope prof("warp_planes", 0.0, (double)a->F * a->H * a->W * 2.0 * a->C, s);
    if (a->C == 1) warp_planes_launch<1, false>(p, a->F, s);
    else if (planar) warp_planes_launch<3, true>(p, a->F, s);
    else warp_planes_launch<3, false>(p, a->F, s);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
