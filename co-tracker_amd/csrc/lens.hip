// Lens distortion on the device (include/ctk.h, "lens"): uint8 pictures resampled between sensor pixels and pinhole pixels, and
// positions carried either way, by the rules stated once in lens_math.h.  One launch each, no atomics; every output element is one
// plain store.
//
// lens_frames  the source position of an output pixel depends on the lens alone, not on the picture.  A workgroup owns a tile of 64 x 16
//              output pixels and one thread 4 consecutive pixels of one row, as in warp.hip; the thread computes the double-precision
//              map of its 4 pixels ONCE -- the closed form, or eight Newton rounds --, keeps the clamped tap offsets, the two
//              fractions and the inside bits in registers and then loops over the pictures of its slice (grid z = Z slices, picture
//              f in slice f % Z; Z = 1 once the tiles alone fill the device, so a 1080p batch pays for its map once).  Taps are byte
//              loads straight from memory at clamped indices: the map is smooth, neighbouring threads read neighbouring bytes, and
//              nothing outside the picture is read under either border.  When dst, its row stride and its frame stride are multiples
//              of 4 bytes the 12 bytes of a thread go out as whole dwords (three for HWC, one per plane for CHW), otherwise as bytes;
//              the Wo % 4 pixels at the end of a row always go bytewise.  No LDS, no scratch; all frame and row offsets are 64-bit.
// lens_points  one thread per point: one 8-byte load, the rule, one 8-byte store and the label byte.  grid (ceil(N / 256), F, G).
#include <float.h>

#include "ctk_common.h"
#include "ctk_profile.h"
#include "lens_math.h"

namespace {

struct LensFramesParams {
  int F, H, W, Ho, Wo, Z;
  long src_frame, src_row, dst_frame, dst_row;
  uint32_t fill;  // fill[0] | fill[1] << 8 | fill[2] << 16
  ctk_lens_rule rule;
  const uint8_t* src;
  uint8_t* dst;
};

constexpr int LENS_PX = 4, LENS_TILE_W = 64, LENS_TILE_H = 16, LENS_FULL_GRID = 1024;

// grid: x = ceil(Wo / 64), y = ceil(Ho / 16), z = Z
template <int LAYOUT, int BORDER, bool DWORDS>
__global__ __launch_bounds__(256) void lens_frames_kernel(LensFramesParams p) {
  const int tid = (int)threadIdx.x;
  const int oy = (int)blockIdx.y * LENS_TILE_H + tid / (LENS_TILE_W / LENS_PX);
  const int ox = (int)blockIdx.x * LENS_TILE_W + (tid % (LENS_TILE_W / LENS_PX)) * LENS_PX;
  if (oy >= p.Ho || ox >= p.Wo) return;
  const int n = p.Wo - ox < LENS_PX ? p.Wo - ox : LENS_PX;  // pixels of this thread that exist
  const long xs = LAYOUT == CTK_INGEST_HWC ? 3 : 1;
  // the map, once: per pixel the offsets of its two tap rows and two tap columns, the fractions, and which taps lie in the picture
  long r0[LENS_PX], r1[LENS_PX];
  int c0[LENS_PX], c1[LENS_PX], frac[LENS_PX], in[LENS_PX];  // in: bit 0..3 = tap 00, 01, 10, 11 inside; bit 4 = the pixel is inside
#pragma unroll
  for (int k = 0; k < LENS_PX; ++k) {
    r0[k] = r1[k] = 0, c0[k] = c1[k] = 0, frac[k] = 0, in[k] = 0;
    if (k >= n) continue;
    int64_t X, Y;
    if (!ctk_lens_coord(&p.rule, ox + k, oy, &X, &Y)) continue;
    const int ix = ctk_lens_whole(X), iy = ctk_lens_whole(Y);
    const int x0 = ctk_warp_clamp(ix, p.W), x1 = ctk_warp_clamp(ix + 1, p.W), y0 = ctk_warp_clamp(iy, p.H), y1 = ctk_warp_clamp(iy + 1, p.H);
    const bool inx0 = x0 == ix, inx1 = x1 == ix + 1, iny0 = y0 == iy, iny1 = y1 == iy + 1;
    r0[k] = (long)y0 * p.src_row, r1[k] = (long)y1 * p.src_row;
    c0[k] = x0 * (int)xs, c1[k] = x1 * (int)xs;
    frac[k] = ctk_lens_frac(X) | ctk_lens_frac(Y) << 8;
    in[k] = 16 | (inx0 && iny0 ? 1 : 0) | (inx1 && iny0 ? 2 : 0) | (inx0 && iny1 ? 4 : 0) | (inx1 && iny1 ? 8 : 0);
  }
  const long splane = LAYOUT == CTK_INGEST_HWC ? 1 : (long)p.H * p.src_row;
  const long dplane = LAYOUT == CTK_INGEST_HWC ? 1 : (long)p.Ho * p.dst_row;
  for (int f = (int)blockIdx.z; f < p.F; f += p.Z) {
    const uint8_t* frame = p.src + (long)f * p.src_frame;
    uint8_t o[3][LENS_PX];
#pragma unroll
    for (int k = 0; k < LENS_PX; ++k) {
      const int fx = frac[k] & 255, fy = frac[k] >> 8;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int fv = (int)((p.fill >> (8 * ch)) & 255u);
        int v = fv;
        if (in[k] & 16) {
          const uint8_t* q = frame + (long)ch * splane;
          int p00 = q[r0[k] + c0[k]], p01 = q[r0[k] + c1[k]], p10 = q[r1[k] + c0[k]], p11 = q[r1[k] + c1[k]];
          if (BORDER == CTK_WARP_FILL)
            p00 = in[k] & 1 ? p00 : fv, p01 = in[k] & 2 ? p01 : fv, p10 = in[k] & 4 ? p10 : fv, p11 = in[k] & 8 ? p11 : fv;
          v = ctk_warp_blend(fx, fy, p00, p01, p10, p11);
        }
        o[ch][k] = (uint8_t)v;
      }
    }
    uint8_t* out = p.dst + (long)f * p.dst_frame + (long)oy * p.dst_row + (long)ox * xs;
    if (DWORDS && n == LENS_PX) {
      if (LAYOUT == CTK_INGEST_HWC) {
        uint32_t* q = reinterpret_cast<uint32_t*>(out);
        q[0] = (uint32_t)o[0][0] | (uint32_t)o[1][0] << 8 | (uint32_t)o[2][0] << 16 | (uint32_t)o[0][1] << 24;
        q[1] = (uint32_t)o[1][1] | (uint32_t)o[2][1] << 8 | (uint32_t)o[0][2] << 16 | (uint32_t)o[1][2] << 24;
        q[2] = (uint32_t)o[2][2] | (uint32_t)o[0][3] << 8 | (uint32_t)o[1][3] << 16 | (uint32_t)o[2][3] << 24;
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          *reinterpret_cast<uint32_t*>(out + (long)ch * dplane) =
              (uint32_t)o[ch][0] | (uint32_t)o[ch][1] << 8 | (uint32_t)o[ch][2] << 16 | (uint32_t)o[ch][3] << 24;
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < LENS_PX; ++k) {
      if (k < n) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[(long)ch * dplane + (long)k * xs] = o[ch][k];
      }
    }
  }
}

template <int LAYOUT, int BORDER>
void lens_frames_launch(const LensFramesParams& p, bool dwords, hipStream_t s) {
  const dim3 grid((unsigned)((p.Wo + LENS_TILE_W - 1) / LENS_TILE_W), (unsigned)((p.Ho + LENS_TILE_H - 1) / LENS_TILE_H), (unsigned)p.Z);
  if (dwords) hipLaunchKernelGGL((lens_frames_kernel<LAYOUT, BORDER, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((lens_frames_kernel<LAYOUT, BORDER, false>), grid, dim3(256), 0, s, p);
}

struct LensPointsParams {
  int N, F;
  long src_group, src_frame, dst_group, dst_frame;
  ctk_lens_rule rule;
  const float* src;
  float* dst;
  int8_t* label;
};

// grid: x = ceil(N / 256), y = F, z = G
__global__ __launch_bounds__(256) void lens_points_kernel(LensPointsParams p) {
  const int n = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (n >= p.N) return;
  const long f = (long)blockIdx.y, g = (long)blockIdx.z;
  const float2 v = *reinterpret_cast<const float2*>(p.src + g * p.src_group + f * p.src_frame + 2l * n);
  uint32_t out[2];
  const int lab = ctk_lens_point(&p.rule, v.x, v.y, out);
  *reinterpret_cast<uint2*>(p.dst + g * p.dst_group + f * p.dst_frame + 2l * n) = make_uint2(out[0], out[1]);
  if (p.label != nullptr) p.label[(g * p.F + f) * p.N + n] = (int8_t)lab;
}

bool lens_ok(const ctk_lens& l, float tol) {
  if (!(l.reserved == 0.0)) return false;
  if (!(tol > 0.0f && tol <= FLT_MAX)) return false;  // (a NaN fails both)
  return ctk_lens_valid(l.sensor, l.ideal, l.k);
}

// bytes from the first to one past the last byte of F pictures
int64_t lens_extent(int F, int H, int W, bool hwc, int64_t frame_stride, int64_t row_stride) {
  return (int64_t)(F - 1) * frame_stride + ((int64_t)H * (hwc ? 1 : 3) - 1) * row_stride + (int64_t)W * (hwc ? 3 : 1);
}

}  // namespace

extern "C" int ctk_lens_frames(const ctk_lens_frames_args* a, void* stream) {
  if (!a || !a->src || !a->dst) return CTK_E_NULL;
  if (a->F < 1 || a->F > 65535 || a->H < 1 || a->H > CTK_INGEST_MAX_SIDE || a->W < 1 || a->W > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->Ho < 1 || a->Ho > CTK_INGEST_MAX_SIDE || a->Wo < 1 || a->Wo > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->layout != CTK_INGEST_HWC && a->layout != CTK_INGEST_CHW) return CTK_E_SHAPE;
  if (a->border != CTK_WARP_FILL && a->border != CTK_WARP_EDGE) return CTK_E_SHAPE;
  if (a->direction != CTK_LENS_TO_IDEAL && a->direction != CTK_LENS_TO_SENSOR) return CTK_E_SHAPE;
  if (a->reserved != 0 || !lens_ok(a->lens, a->tol)) return CTK_E_SHAPE;
  const bool hwc = a->layout == CTK_INGEST_HWC;
  const int64_t big = (int64_t)1 << 40;
  const int64_t sizes[2][2] = {{a->H, a->W}, {a->Ho, a->Wo}};
  const int64_t strides[2][2] = {{a->src_frame_stride, a->src_row_stride}, {a->dst_frame_stride, a->dst_row_stride}};
  for (int k = 0; k < 2; ++k) {
    const int64_t frame = strides[k][0], row = strides[k][1];
    if (row < sizes[k][1] * (hwc ? 3 : 1) || row > big || frame > big) return CTK_E_SHAPE;
    if (frame < row * sizes[k][0] * (hwc ? 1 : 3)) return CTK_E_SHAPE;
  }
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(a->src), d0 = reinterpret_cast<uintptr_t>(a->dst);
  const uintptr_t s1 = s0 + (uintptr_t)lens_extent(a->F, a->H, a->W, hwc, a->src_frame_stride, a->src_row_stride);
  const uintptr_t d1 = d0 + (uintptr_t)lens_extent(a->F, a->Ho, a->Wo, hwc, a->dst_frame_stride, a->dst_row_stride);
  if (s0 < d1 && d0 < s1) return CTK_E_SHAPE;  // a resampling cannot run in place
  hipStream_t s = static_cast<hipStream_t>(stream);
  LensFramesParams p;
  p.F = a->F, p.H = a->H, p.W = a->W, p.Ho = a->Ho, p.Wo = a->Wo;
  p.src_frame = (long)a->src_frame_stride, p.src_row = (long)a->src_row_stride;
  p.dst_frame = (long)a->dst_frame_stride, p.dst_row = (long)a->dst_row_stride;
  p.fill = (uint32_t)a->fill[0] | (uint32_t)a->fill[1] << 8 | (uint32_t)a->fill[2] << 16;
  // an output pixel of the pinhole picture is an ideal position: the point rule of the other direction
  ctk_lens_prepare(a->lens.sensor, a->lens.ideal, a->lens.k, a->direction == CTK_LENS_TO_IDEAL ? CTK_LENS_TO_SENSOR : CTK_LENS_TO_IDEAL,
                   a->tol, &p.rule);
  p.src = a->src, p.dst = a->dst;
  // slices of pictures over grid z only as far as a small picture needs them to fill the device
  const long tiles = (long)((a->Wo + LENS_TILE_W - 1) / LENS_TILE_W) * ((a->Ho + LENS_TILE_H - 1) / LENS_TILE_H);
  const long want = tiles >= LENS_FULL_GRID ? 1 : (LENS_FULL_GRID + tiles - 1) / tiles;
  p.Z = (int)(want < a->F ? want : a->F);
  // whole dwords: every 4-pixel group of every row of every picture (and plane) then starts on a 4-byte multiple of the base
  const bool dwords = (d0 & 3u) == 0 && a->dst_row_stride % 4 == 0 && (a->F == 1 || a->dst_frame_stride % 4 == 0);
  {
    CtkProfScope prof("lens_frames", 0.0, (double)a->F * a->Ho * a->Wo * 6.0, s);
    if (hwc) {
      if (a->border == CTK_WARP_FILL) lens_frames_launch<CTK_INGEST_HWC, CTK_WARP_FILL>(p, dwords, s);
      else lens_frames_launch<CTK_INGEST_HWC, CTK_WARP_EDGE>(p, dwords, s);
    } else {
      if (a->border == CTK_WARP_FILL) lens_frames_launch<CTK_INGEST_CHW, CTK_WARP_FILL>(p, dwords, s);
      else lens_frames_launch<CTK_INGEST_CHW, CTK_WARP_EDGE>(p, dwords, s);
    }
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

extern "C" int ctk_lens_points(const ctk_lens_points_args* a, void* stream) {
  if (!a || !a->src || !a->dst) return CTK_E_NULL;
  if (a->G < 1 || a->G > 65535 || a->F < 1 || a->F > 65535 || a->N < 1 || a->N > (1 << 20)) return CTK_E_SHAPE;
  if (a->direction != CTK_LENS_TO_IDEAL && a->direction != CTK_LENS_TO_SENSOR) return CTK_E_SHAPE;
  if (a->reserved != 0 || !lens_ok(a->lens, a->tol)) return CTK_E_SHAPE;
  const int64_t big = (int64_t)1 << 40;
  const int64_t strides[2][2] = {{a->src_group_stride, a->src_frame_stride}, {a->dst_group_stride, a->dst_frame_stride}};
  int64_t ext[2];
  for (int k = 0; k < 2; ++k) {
    const int64_t group = strides[k][0], frame = strides[k][1];
    if (frame < 2 * (int64_t)a->N || frame > big || group > big || group < frame * a->F) return CTK_E_SHAPE;
    ext[k] = 4 * ((a->G - 1) * group + (a->F - 1) * frame + 2 * (int64_t)a->N);
  }
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(a->src), d0 = reinterpret_cast<uintptr_t>(a->dst);
  const uintptr_t s1 = s0 + (uintptr_t)ext[0], d1 = d0 + (uintptr_t)ext[1];
  const bool in_place = s0 == d0 && a->src_group_stride == a->dst_group_stride && a->src_frame_stride == a->dst_frame_stride;
  if (!in_place && s0 < d1 && d0 < s1) return CTK_E_SHAPE;  // an element is read and written by its own thread, or the ranges are apart
  if (a->label) {
    const uintptr_t l0 = reinterpret_cast<uintptr_t>(a->label), l1 = l0 + (uintptr_t)((int64_t)a->G * a->F * a->N);
    if ((l0 < s1 && s0 < l1) || (l0 < d1 && d0 < l1)) return CTK_E_SHAPE;
  }
  if ((s0 & 7u) != 0 || (d0 & 7u) != 0) return CTK_E_ALIGN;
  for (int k = 0; k < 2; ++k)
    if (strides[k][0] % 2 != 0 || strides[k][1] % 2 != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  LensPointsParams p;
  p.N = a->N, p.F = a->F;
  p.src_group = (long)a->src_group_stride, p.src_frame = (long)a->src_frame_stride;
  p.dst_group = (long)a->dst_group_stride, p.dst_frame = (long)a->dst_frame_stride;
  ctk_lens_prepare(a->lens.sensor, a->lens.ideal, a->lens.k, a->direction, a->tol, &p.rule);
  p.src = a->src, p.dst = a->dst, p.label = a->label;
  {
    CtkProfScope prof("lens_points", 0.0, (double)a->G * a->F * a->N * 17.0, s);
    hipLaunchKernelGGL(lens_points_kernel, dim3((unsigned)((a->N + 255) / 256), (unsigned)a->F, (unsigned)a->G), dim3(256), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
