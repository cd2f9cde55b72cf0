// Stabilise frames on the device (include/ctk.h, "warp frames"): the path rule that turns per-frame camera motions into corrections,
// and the resampling of uint8 pictures under a 2 x 3 matrix, by the rules stated once in warp_math.h.  One launch each, no
// atomics; every output element is one plain store.
//
// smooth_path  one thread per group walks its F frames in order: the state (six doubles) is read once, stepped in registers and
//              written back once.  The work is a few hundred double operations per group: latency, not throughput.
// warp_frames  grid z is the picture, a workgroup owns a tile of 64 x 16 output pixels and one thread makes 4 consecutive pixels of one
//              row for all three channels.  The workgroup stages the source bounding box of its tile (a few pixels larger than the
//              tile for the near-identity matrices a stabiliser produces) into 16 KiB of LDS with whole-dword loads and samples from
//              there; a box that does not fit is sampled from memory with byte loads.  A thread fixes the matrix to Q24 once and
//              steps X, Y by c00, c10 from pixel to pixel (exact, so the same bits as the closed form); taps are read at clamped
//              indices -- nothing outside the picture is read with either border; CTK_WARP_FILL then replaces a tap that lay outside
//              by fill[c].  When dst, its row stride and its frame stride are multiples of 4 bytes the 12 bytes of a thread go out as
//              whole dwords (three for HWC, one per plane for CHW), otherwise as bytes; the W % 4 pixels at the end of a row always
//              go bytewise.  No atomics, no scratch; all frame and row offsets are 64-bit.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "warp_math.h"

namespace {

struct PathParams {
  int G, F;
  float alpha;
  const float* motion;
  const float* post;
  double* state;
  float* warp;
};

// grid: x = ceil(G / 64)
__global__ __launch_bounds__(64) void smooth_path_kernel(PathParams p) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= p.G) return;
  double W[6];
  double* st = p.state + (long)g * 6;
#pragma unroll
  for (int i = 0; i < 6; ++i) W[i] = st[i];
  float post[6];
  const bool have_post = p.post != nullptr;
#pragma unroll
  for (int i = 0; i < 6; ++i) post[i] = have_post ? p.post[i] : 0.0f;
  for (int f = 0; f < p.F; ++f) {
    const float* mo = p.motion + ((long)g * p.F + f) * 6;
    float m[6], o[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = mo[i];
    if (have_post) ctk_path_step(m, p.alpha, post, W, o);  // (two calls: neither takes the address of `post` conditionally)
    else ctk_path_step(m, p.alpha, nullptr, W, o);
    float* out = p.warp + ((long)g * p.F + f) * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = o[i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) st[i] = W[i];
}

struct WarpParams {
  int H, W;
  long src_frame, src_row, dst_frame, dst_row;
  uint32_t fill;  // fill[0] | fill[1] << 8 | fill[2] << 16
  const float* matrices;
  const uint8_t* src;
  uint8_t* dst;
};

constexpr int WARP_PX = 4;

// a tap straight from memory: byte loads
template <int LAYOUT>
struct WarpDirect {
  const uint8_t* frame;
  long row, plane;
  __device__ __forceinline__ int operator()(int ch, int y, int x) const {
    return LAYOUT == CTK_INGEST_HWC ? frame[(long)y * row + (long)x * 3 + ch] : frame[(long)ch * plane + (long)y * row + x];
  }
};

// The 4 output pixels (ox .. ox + 3, oy) of picture `pic`: coordinates stepped from the closed form, taps through `fetch` at clamped
// indices, the 12 bytes stored as dwords or bytes.  GUARD: pixels beyond W fetch nothing (a fetch that cannot serve every index).
template <int LAYOUT, int BORDER, bool DWORDS, bool GUARD, typename Fetch>
__device__ __forceinline__ void warp_pixels(const WarpParams& p, int pic, int ox, int oy, const int64_t* c, const Fetch& fetch) {
  int64_t X = ctk_warp_coord(c, ox, oy), Y = ctk_warp_coord(c + 3, ox, oy);
  const long xs = LAYOUT == CTK_INGEST_HWC ? 3 : 1;
  const int n = p.W - ox < WARP_PX ? p.W - ox : WARP_PX;  // pixels of this thread that exist
  uint8_t o[3][WARP_PX];
#pragma unroll
  for (int k = 0; k < WARP_PX; ++k) {
    const int ix = ctk_warp_whole(X), iy = ctk_warp_whole(Y), fx = ctk_warp_frac(X), fy = ctk_warp_frac(Y);
    X += c[0], Y += c[3];
    const int x0 = ctk_warp_clamp(ix, p.W), x1 = ctk_warp_clamp(ix + 1, p.W), y0 = ctk_warp_clamp(iy, p.H), y1 = ctk_warp_clamp(iy + 1, p.H);
    const bool inx0 = x0 == ix, inx1 = x1 == ix + 1, iny0 = y0 == iy, iny1 = y1 == iy + 1;
    if (GUARD && k >= n) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch][k] = 0;
      continue;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int p00 = fetch(ch, y0, x0), p01 = fetch(ch, y0, x1), p10 = fetch(ch, y1, x0), p11 = fetch(ch, y1, x1);
      if (BORDER == CTK_WARP_FILL) {
        const int fv = (int)((p.fill >> (8 * ch)) & 255u);
        p00 = inx0 && iny0 ? p00 : fv, p01 = inx1 && iny0 ? p01 : fv, p10 = inx0 && iny1 ? p10 : fv, p11 = inx1 && iny1 ? p11 : fv;
      }
      o[ch][k] = (uint8_t)ctk_warp_blend(fx, fy, p00, p01, p10, p11);
    }
  }
  uint8_t* out = p.dst + (long)pic * p.dst_frame + (long)oy * p.dst_row + (long)ox * xs;
  const long dplane = LAYOUT == CTK_INGEST_HWC ? 1 : (long)p.H * p.dst_row;
  if (DWORDS && n == WARP_PX) {
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
    return;
  }
#pragma unroll
  for (int k = 0; k < WARP_PX; ++k) {
    if (k < n) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out[(long)ch * dplane + (long)k * xs] = o[ch][k];
    }
  }
}

__device__ __forceinline__ void warp_matrix(const WarpParams& p, int pic, int64_t* c) {
  const float* mp = p.matrices + (long)pic * 6;
  float m[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) m[k] = mp[k];
  ctk_warp_fix(m, c);
}

// A workgroup owns a tile of 64 x 16 output pixels, stages the source bounding box of the tile -- clamped into the picture, so every clamped tap index lies in
// it -- into LDS, whole dwords where a box row allows and bytes at its two ends (nothing outside the box is read), and samples from
// LDS.  A box row keeps its phase (address & 3) in LDS, so the dwords go in aligned.  When the box does not fit WARP_LDS_BYTES the
// workgroup samples from memory (WarpDirect).
constexpr int WARP_TILE_W = 64, WARP_TILE_H = 16, WARP_LDS_BYTES = 16384;

template <int LAYOUT>
struct WarpStaged {
  const uint8_t* lds;
  int bx0, by0, bh, pitch;
  unsigned base_lo, row_lo;  // (address of box row 0) & 3, row stride & 3
  int H;
  __device__ __forceinline__ int operator()(int ch, int y, int x) const {
    const int r = LAYOUT == CTK_INGEST_HWC ? y - by0 : ch * bh + (y - by0);
    const unsigned g = LAYOUT == CTK_INGEST_HWC ? (unsigned)(y - by0) : (unsigned)(ch * H + (y - by0));  // rows from box row 0 in memory
    const unsigned ph = (base_lo + g * row_lo) & 3u;
    return lds[r * pitch + (int)ph + (LAYOUT == CTK_INGEST_HWC ? (x - bx0) * 3 + ch : x - bx0)];
  }
};

// grid: x = ceil(W / 64), y = ceil(H / 16), z = picture
template <int LAYOUT, int BORDER, bool DWORDS>
__global__ __launch_bounds__(256) void warp_frames_kernel(WarpParams p) {
  __shared__ uint32_t lds[WARP_LDS_BYTES / 4];
  const int tid = (int)threadIdx.x, pic = (int)blockIdx.z;
  const int tx0 = (int)blockIdx.x * WARP_TILE_W, ty0 = (int)blockIdx.y * WARP_TILE_H;
  const int tx1 = min(tx0 + WARP_TILE_W, p.W) - 1, ty1 = min(ty0 + WARP_TILE_H, p.H) - 1;  // the tile's last pixel
  int64_t c[6];
  warp_matrix(p, pic, c);
  // the box: an affine coordinate takes its extremes on the tile's corners
  const int64_t xa = ctk_warp_coord(c, tx0, ty0), xb = ctk_warp_coord(c, tx1, ty0), xc = ctk_warp_coord(c, tx0, ty1), xd = ctk_warp_coord(c, tx1, ty1);
  const int64_t ya = ctk_warp_coord(c + 3, tx0, ty0), yb = ctk_warp_coord(c + 3, tx1, ty0), yc = ctk_warp_coord(c + 3, tx0, ty1),
                yd = ctk_warp_coord(c + 3, tx1, ty1);
  const int bx0 = ctk_warp_clamp(ctk_warp_whole(min(min(xa, xb), min(xc, xd))), p.W);
  const int bx1 = ctk_warp_clamp(ctk_warp_whole(max(max(xa, xb), max(xc, xd))) + 1, p.W);
  const int by0 = ctk_warp_clamp(ctk_warp_whole(min(min(ya, yb), min(yc, yd))), p.H);
  const int by1 = ctk_warp_clamp(ctk_warp_whole(max(max(ya, yb), max(yc, yd))) + 1, p.H);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const int row_bytes = LAYOUT == CTK_INGEST_HWC ? bw * 3 : bw, rows = LAYOUT == CTK_INGEST_HWC ? bh : bh * 3;
  const int pitch = (row_bytes + 6) & ~3;  // a phase of up to 3 bytes in front, rounded up to dwords
  const bool staged = (long)rows * pitch <= WARP_LDS_BYTES;
  const uint8_t* frame = p.src + (long)pic * p.src_frame;
  const int oy = ty0 + tid / (WARP_TILE_W / WARP_PX), ox = tx0 + (tid % (WARP_TILE_W / WARP_PX)) * WARP_PX;
  const bool mine = oy < p.H && ox < p.W;
  if (!staged) {
    const WarpDirect<LAYOUT> fetch = {frame, p.src_row, (long)p.H * p.src_row};
    if (mine) warp_pixels<LAYOUT, BORDER, DWORDS, true>(p, pic, ox, oy, c, fetch);
    return;
  }
  const uint8_t* box = frame + (long)by0 * p.src_row + (long)bx0 * (LAYOUT == CTK_INGEST_HWC ? 3 : 1);  // box row 0 (of plane 0)
  const int nd = pitch / 4;
  for (int idx = tid; idx < rows * nd; idx += 256) {
    const int r = idx / nd, d = idx - r * nd;
    const long g = LAYOUT == CTK_INGEST_HWC ? r : (long)(r / bh) * p.H + (r % bh);  // memory rows from box row 0
    const uint8_t* b0 = box + g * p.src_row;                                         // the first and one past the last byte of the box row
    const uint8_t* b1 = b0 + row_bytes;
    const uint8_t* q = b0 - (reinterpret_cast<uintptr_t>(b0) & 3u) + 4 * d;          // an aligned dword of memory
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
  const WarpStaged<LAYOUT> fetch = {reinterpret_cast<const uint8_t*>(lds), bx0, by0, bh, pitch,
                                    (unsigned)(reinterpret_cast<uintptr_t>(box) & 3u), (unsigned)(p.src_row & 3), p.H};
  if (mine) warp_pixels<LAYOUT, BORDER, DWORDS, true>(p, pic, ox, oy, c, fetch);
}

template <int LAYOUT, int BORDER>
void warp_launch(const WarpParams& p, int F, bool dwords, hipStream_t s) {
  const dim3 grid((unsigned)((p.W + WARP_TILE_W - 1) / WARP_TILE_W), (unsigned)((p.H + WARP_TILE_H - 1) / WARP_TILE_H), (unsigned)F);
  if (dwords) hipLaunchKernelGGL((warp_frames_kernel<LAYOUT, BORDER, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((warp_frames_kernel<LAYOUT, BORDER, false>), grid, dim3(256), 0, s, p);
}
#ifdef CTK_DEV
// The direct form, kept in the dev library only (DESIGN.md has the measurement that decided against it): ingest.hip's shape, one
// thread per 4 output pixels of a row over a flat grid, every tap a byte load from memory; no LDS.
// grid: x = ceil(H * ceil(W / 4) / 256), y = picture
template <int LAYOUT, int BORDER, bool DWORDS>
__global__ __launch_bounds__(256) void warp_frames_direct_kernel(WarpParams p) {
  const int wq = (p.W + WARP_PX - 1) / WARP_PX;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)p.H * wq) return;
  const int oy = (int)(i / wq), ox = (int)(i - (long)oy * wq) * WARP_PX;
  const int pic = (int)blockIdx.y;
  int64_t c[6];
  warp_matrix(p, pic, c);
  const WarpDirect<LAYOUT> fetch = {p.src + (long)pic * p.src_frame, p.src_row, (long)p.H * p.src_row};
  warp_pixels<LAYOUT, BORDER, DWORDS, false>(p, pic, ox, oy, c, fetch);
}

template <int LAYOUT, int BORDER>
void warp_launch_direct(const WarpParams& p, int F, bool dwords, hipStream_t s) {
  const unsigned blocks = (unsigned)(((long)p.H * ((p.W + WARP_PX - 1) / WARP_PX) + 255) / 256);
  if (dwords) hipLaunchKernelGGL((warp_frames_direct_kernel<LAYOUT, BORDER, true>), dim3(blocks, (unsigned)F), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((warp_frames_direct_kernel<LAYOUT, BORDER, false>), dim3(blocks, (unsigned)F), dim3(256), 0, s, p);
}

#endif

// elements from the first to one past the last byte of F pictures
int64_t warp_extent(int F, int H, int W, bool hwc, int64_t frame_stride, int64_t row_stride) {
  return (int64_t)(F - 1) * frame_stride + ((int64_t)H * (hwc ? 1 : 3) - 1) * row_stride + (int64_t)W * (hwc ? 3 : 1);
}

}  // namespace

extern "C" int ctk_smooth_path(const ctk_smooth_path_args* a, void* stream) {
  if (!a || !a->motion || !a->state || !a->warp) return CTK_E_NULL;
  if (a->G < 1 || a->G > 65535 || a->F < 1 || a->F > 65535 || a->reserved != 0) return CTK_E_SHAPE;
  if (!(a->alpha >= 0.0f && a->alpha <= 1.0f)) return CTK_E_SHAPE;  // (a NaN fails both)
  if ((reinterpret_cast<uintptr_t>(a->state) & 7u) != 0) return CTK_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(a->motion) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->warp) & 3u) != 0) return CTK_E_ALIGN;
  if (a->post && (reinterpret_cast<uintptr_t>(a->post) & 3u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PathParams p;
  p.G = a->G, p.F = a->F, p.alpha = a->alpha;
  p.motion = a->motion, p.post = a->post, p.state = a->state, p.warp = a->warp;
  {
    CtkProfScope prof("smooth_path", 0.0, (double)a->G * (a->F * 48.0 + 96.0), s);
    hipLaunchKernelGGL(smooth_path_kernel, dim3((unsigned)((a->G + 63) / 64)), dim3(64), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

namespace {

// the checks and the launch of ctk_warp_frames; `direct` (dev library only): the kernel without LDS
int warp_run(const ctk_warp_args* a, void* stream, bool direct) {
  if (!a || !a->matrices || !a->src || !a->dst) return CTK_E_NULL;
  if (a->F < 1 || a->F > 65535 || a->H < 1 || a->H > CTK_INGEST_MAX_SIDE || a->W < 1 || a->W > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->layout != CTK_INGEST_HWC && a->layout != CTK_INGEST_CHW) return CTK_E_SHAPE;
  if (a->border != CTK_WARP_FILL && a->border != CTK_WARP_EDGE) return CTK_E_SHAPE;
  if (a->reserved != 0) return CTK_E_SHAPE;
  const bool hwc = a->layout == CTK_INGEST_HWC;
  const int64_t big = (int64_t)1 << 40;
  const int64_t strides[2][2] = {{a->src_frame_stride, a->src_row_stride}, {a->dst_frame_stride, a->dst_row_stride}};
  for (int k = 0; k < 2; ++k) {
    const int64_t frame = strides[k][0], row = strides[k][1];
    if (row < (int64_t)a->W * (hwc ? 3 : 1) || row > big || frame > big) return CTK_E_SHAPE;
    if (frame < row * a->H * (hwc ? 1 : 3)) return CTK_E_SHAPE;
  }
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(a->src), d0 = reinterpret_cast<uintptr_t>(a->dst);
  const uintptr_t s1 = s0 + (uintptr_t)warp_extent(a->F, a->H, a->W, hwc, a->src_frame_stride, a->src_row_stride);
  const uintptr_t d1 = d0 + (uintptr_t)warp_extent(a->F, a->H, a->W, hwc, a->dst_frame_stride, a->dst_row_stride);
  if (s0 < d1 && d0 < s1) return CTK_E_SHAPE;  // a warp cannot run in place
  if ((reinterpret_cast<uintptr_t>(a->matrices) & 3u) != 0) return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  WarpParams p;
  p.H = a->H, p.W = a->W;
  p.src_frame = (long)a->src_frame_stride, p.src_row = (long)a->src_row_stride;
  p.dst_frame = (long)a->dst_frame_stride, p.dst_row = (long)a->dst_row_stride;
  p.fill = (uint32_t)a->fill[0] | (uint32_t)a->fill[1] << 8 | (uint32_t)a->fill[2] << 16;
  p.matrices = a->matrices, p.src = a->src, p.dst = a->dst;
  // whole dwords: every 4-pixel group of every row of every picture (and plane) then starts on a 4-byte multiple of the base
  const bool dwords = (d0 & 3u) == 0 && a->dst_row_stride % 4 == 0 && (a->F == 1 || a->dst_frame_stride % 4 == 0);
  {
    CtkProfScope prof("warp_frames", 0.0, (double)a->F * a->H * a->W * 6.0, s);
#ifdef CTK_DEV
    if (direct) {
      if (hwc) {
        if (a->border == CTK_WARP_FILL) warp_launch_direct<CTK_INGEST_HWC, CTK_WARP_FILL>(p, a->F, dwords, s);
        else warp_launch_direct<CTK_INGEST_HWC, CTK_WARP_EDGE>(p, a->F, dwords, s);
      } else {
        if (a->border == CTK_WARP_FILL) warp_launch_direct<CTK_INGEST_CHW, CTK_WARP_FILL>(p, a->F, dwords, s);
        else warp_launch_direct<CTK_INGEST_CHW, CTK_WARP_EDGE>(p, a->F, dwords, s);
      }
    } else
#endif
    if (hwc) {
      if (a->border == CTK_WARP_FILL) warp_launch<CTK_INGEST_HWC, CTK_WARP_FILL>(p, a->F, dwords, s);
      else warp_launch<CTK_INGEST_HWC, CTK_WARP_EDGE>(p, a->F, dwords, s);
    } else {
      if (a->border == CTK_WARP_FILL) warp_launch<CTK_INGEST_CHW, CTK_WARP_FILL>(p, a->F, dwords, s);
      else warp_launch<CTK_INGEST_CHW, CTK_WARP_EDGE>(p, a->F, dwords, s);
    }
  }
  (void)direct;
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_warp_frames(const ctk_warp_args* a, void* stream) { return warp_run(a, stream, false); }

#ifdef CTK_DEV
// dev tools (make dev; tools/bench_stream_stabilize.py, tests/test_gpu_warp.py; not part of include/ctk.h): ctk_warp_frames through
// the direct kernel -- the same arguments, refusals and bytes.
extern "C" int ctk_debug_warp_frames_direct(const ctk_warp_args* a, void* stream) { return warp_run(a, stream, true); }
#endif
