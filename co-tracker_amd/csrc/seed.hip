// The best-textured pixel of every cell of a grid over one model-resolution frame, in one launch (include/ctk.h, "seed points"):
// where a tracker should put a new point.  The score is floor(2 lambda_min) of the structure tensor of the luminance, in integer
// arithmetic stated once in seed_math.h; the cell of a pixel is the cell ctk_stream_health counts a point at that position in.
//
// One workgroup of 256 threads per cell.  Two threads find the cell's candidate rectangle (the cell rule is monotone: a binary
// search per edge); the workgroup then walks it in tiles of 32 x 8 candidates, one per thread.  Per tile: the luminance of the tile
// plus an r+1 halo goes to LDS (three coalesced row reads per pixel, coordinates clamped into the image: nothing outside the frame is
// ever read, and the clamp IS the replicated border of the gradient), then the gradients of the tile plus an r halo, gx and gy
// packed in one dword and zero outside the image, then every thread sums its (2r+1)^2 window -- one LDS dword per term, rows of 32
// consecutive lanes: no bank conflicts -- and keeps the best key (score, -py, -px) it has seen.  A tree reduction over the 256 keys
// ends the walk; thread 0 stores the cell's three output integers.  Every output element is written by that plain store: no fill,
// no atomics, and the maximum of a set of distinct integer keys does not depend on the order in which it is taken.
#include "ctk_common.h"
#include "seed_math.h"

namespace {

constexpr int SEED_TW = 32, SEED_TH = 8;                   // candidates per tile
constexpr int SEED_LW = SEED_TW + 2 * (CTK_SEED_RADIUS_MAX + 1);  // 48: luminance tile with its r+1 halo
constexpr int SEED_LH = SEED_TH + 2 * (CTK_SEED_RADIUS_MAX + 1);  // 24
constexpr int SEED_GW = SEED_TW + 2 * CTK_SEED_RADIUS_MAX;        // 46: gradient tile with its r halo
constexpr int SEED_GH = SEED_TH + 2 * CTK_SEED_RADIUS_MAX;        // 22
constexpr int SEED_CELLS_MAX = 65536;

struct SeedParams {
  const float* frame;
  int h, w, radius, margin, inset, min_score;
  float x_lo, x_hi, y_lo, y_hi;
  int gh, gw;
  float inv_cw, inv_ch;
};

__global__ __launch_bounds__(256) void seed_points_kernel(SeedParams p, int32_t* __restrict__ seeds) {
  __shared__ int lum[SEED_LH * SEED_LW];
  __shared__ int grad[SEED_GH * SEED_GW];
  __shared__ int64_t keys[256];
  __shared__ int rect[4];
  const int tid = (int)threadIdx.x;
  const int cell = (int)blockIdx.x;
  const int cy = cell / p.gw, cx = cell - cy * p.gw;
  if (tid == 0) ctk_seed_candidates(cx, p.x_lo, p.x_hi, p.inv_cw, p.gw, p.w, p.margin, p.inset, &rect[0], &rect[1]);
  if (tid == 64) ctk_seed_candidates(cy, p.y_lo, p.y_hi, p.inv_ch, p.gh, p.h, p.margin, p.inset, &rect[2], &rect[3]);
  __syncthreads();
  const int X0 = rect[0], X1 = rect[1], Y0 = rect[2], Y1 = rect[3];  // (block-uniform)
  const int r = p.radius;
  const int tx = tid & (SEED_TW - 1), ty = tid / SEED_TW;
  const long plane = (long)p.h * p.w;
  int64_t best = -1;
  for (int ty0 = Y0; ty0 <= Y1; ty0 += SEED_TH) {
    const int th = min(SEED_TH, Y1 - ty0 + 1);
    for (int tx0 = X0; tx0 <= X1; tx0 += SEED_TW) {
      const int tw = min(SEED_TW, X1 - tx0 + 1);
      const int lw = tw + 2 * r + 2, lh = th + 2 * r + 2;  // <= SEED_LW, SEED_LH
      const int gw_ = tw + 2 * r, gh_ = th + 2 * r;        // <= SEED_GW, SEED_GH
      __syncthreads();  // the previous tile's sums have read grad; (first tile: rect)
      for (int i = tid; i < lw * lh; i += 256) {
        const int ly = i / lw, lx = i - ly * lw;
        const int y = min(max(ty0 - r - 1 + ly, 0), p.h - 1), x = min(max(tx0 - r - 1 + lx, 0), p.w - 1);
        const float* q = p.frame + (long)y * p.w + x;
        lum[ly * SEED_LW + lx] = ctk_seed_luma(q[0], q[plane], q[2 * plane]);
      }
      __syncthreads();
      for (int i = tid; i < gw_ * gh_; i += 256) {
        const int gy_ = i / gw_, gx_ = i - gy_ * gw_;
        const int y = ty0 - r + gy_, x = tx0 - r + gx_;
        int v = 0;
        if (y >= 0 && y < p.h && x >= 0 && x < p.w) {
          const int* c = lum + (gy_ + 1) * SEED_LW + gx_ + 1;  // lum holds clamped coordinates: the neighbours past a border are the border
          const int dx = c[1] - c[-1], dy = c[SEED_LW] - c[-SEED_LW];
          v = (dx & 0xffff) | (int)((unsigned)dy << 16);
        }
        grad[gy_ * SEED_GW + gx_] = v;
      }
      __syncthreads();
      if (tx < tw && ty < th) {
        int a = 0, b = 0, c = 0;
        for (int dy = 0; dy <= 2 * r; ++dy) {
          const int* row = grad + (ty + dy) * SEED_GW + tx;
          for (int dx = 0; dx <= 2 * r; ++dx) {
            const int v = row[dx];
            const int gx = (int)(short)(v & 0xffff), gy = v >> 16;
            a += gx * gx, b += gx * gy, c += gy * gy;
          }
        }
        const int64_t k = ctk_seed_key(ctk_seed_score(a, b, c), ty0 + ty, tx0 + tx);
        best = k > best ? k : best;
      }
    }
  }
  keys[tid] = best;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const int64_t o = keys[tid + s];
      if (o > keys[tid]) keys[tid] = o;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t k = keys[0];
    int32_t* out = seeds + (long)cell * 3;
    if (k < 0 || ctk_seed_key_score(k) < p.min_score) {
      out[0] = -1, out[1] = -1, out[2] = -1;
    } else {
      out[0] = ctk_seed_key_px(k), out[1] = ctk_seed_key_py(k), out[2] = ctk_seed_key_score(k);
    }
  }
}

}  // namespace

extern "C" int ctk_seed_points(const ctk_seed_args* a, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->frame || !a->seeds) return CTK_E_NULL;
  if (a->h < 1 || a->w < 1 || a->h > CTK_INGEST_MAX_SIDE || a->w > CTK_INGEST_MAX_SIDE) return CTK_E_SHAPE;
  if (a->radius < 1 || a->radius > CTK_SEED_RADIUS_MAX || a->margin < 0 || a->inset < 0 || a->min_score < 0) return CTK_E_SHAPE;
  if (a->gh <= 0 || a->gw <= 0 || (long)a->gh * a->gw > SEED_CELLS_MAX || a->reserved != 0) return CTK_E_SHAPE;
  if (!std::isfinite(a->x_lo) || !std::isfinite(a->x_hi) || !std::isfinite(a->y_lo) || !std::isfinite(a->y_hi)) return CTK_E_SHAPE;
  if (a->x_hi <= a->x_lo || a->y_hi <= a->y_lo) return CTK_E_SHAPE;
  if (!std::isfinite(a->inv_cw) || !std::isfinite(a->inv_ch) || !(a->inv_cw > 0.0f) || !(a->inv_ch > 0.0f)) return CTK_E_SHAPE;
  if ((reinterpret_cast<uintptr_t>(a->frame) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->seeds) & 3u) != 0) return CTK_E_ALIGN;
  SeedParams p;
  p.frame = a->frame, p.h = a->h, p.w = a->w, p.radius = a->radius, p.margin = a->margin, p.inset = a->inset, p.min_score = a->min_score;
  p.x_lo = a->x_lo, p.x_hi = a->x_hi, p.y_lo = a->y_lo, p.y_hi = a->y_hi;
  p.gh = a->gh, p.gw = a->gw, p.inv_cw = a->inv_cw, p.inv_ch = a->inv_ch;
  hipLaunchKernelGGL(seed_points_kernel, dim3((unsigned)(a->gh * a->gw)), dim3(256), 0, static_cast<hipStream_t>(stream), p, a->seeds);
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
