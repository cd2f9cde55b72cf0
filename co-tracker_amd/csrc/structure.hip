// Points added to a 3-D structure on the device (include/ctk.h, "fit structure"): per (group, slot) the tracked positions on F localised
// frames become a 3-D point in the structure's unit, by the rules of structure_math.h (and, through it, resection_math.h and
// pose_math.h); the old structure is carried along and everything is restated in the camera of one of the frames.  One launch, no
// atomics, no workspace; every output element is one plain store; every input is only read.
//
// One workgroup of 64 threads (one wave) owns 64 slots of one group: N_out = 1024 spreads over 16 workgroups.
// setup     threads j, j + 64, ... < F validate view j (twelve floats, four polar steps) and publish (R | t), the centre and whether
//           the view counts in LDS: 15 doubles and a byte per view, 30.25 KiB at 256 views.  Behind the one barrier the views are read only.
// slots     a thread per slot walks the views in ascending j, five times: the start, three rounds, the final classification with the
//           parallax test.  Every walk reads the positions again from global memory (float2, coalesced across the slots of a row;
//           the poses are LDS broadcasts): no thread keeps F positions.
// origin    thread 0 of the first workgroup of a group writes origin_out.
#include "ctk_common.h"
#include "ctk_profile.h"
#include "fit_device.h"  // fit_scale_ok, fit_finite
#include "structure_math.h"

namespace {

constexpr int ST_BLOCK = 64;

struct StructureParams {
  int G, N, N_out, R, f0, F, into, source_frame, min_views, refine;
  float sx, sy, thresh, tol, min_sin2;
  CtkPoseCam cam;
  const float* hc;
  const uint8_t* visible;
  const float* hv;
  const float* hf;
  const int32_t* first_row;
  const float* pose;
  const int32_t* pose_stats;
  const float* structure_in;
  const int8_t* valid_in;
  const float* origin_in;
  float* points;
  int8_t* label;
  float* error;
  int32_t* stats;
  float* origin_out;
};

// grid: x = a block of ST_BLOCK slots, y = group
__global__ __launch_bounds__(ST_BLOCK) void fit_structure_kernel(StructureParams p) {
  __shared__ __attribute__((aligned(16))) CtkStructureView views[CTK_STRUCTURE_VIEWS_MAX];  // 120 bytes each
  __shared__ __attribute__((aligned(16))) uint8_t counts[CTK_STRUCTURE_VIEWS_MAX];
  const int tid = (int)threadIdx.x;
  const long g = (long)blockIdx.y;
  const int n = (int)blockIdx.x * ST_BLOCK + tid;
  const int F = p.F;

  // 1. the views
  for (int j = tid; j < F; j += ST_BLOCK) {
    const float* mp = p.pose + (g * F + j) * 12;
    float m12[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m12[i] = mp[i];
    const bool stats_ok = p.pose_stats == nullptr || p.pose_stats[(g * F + j) * 4 + 2] >= 0;
    CtkStructureView v;
    const bool ok = ctk_structure_view(m12, stats_ok, &v);
    views[j] = v;
    counts[j] = ok ? 1 : 0;
  }
  __syncthreads();

  const bool into_counts = p.into >= 0 && counts[p.into] != 0;  // (the same in every thread)
  const bool no_structure = p.into >= 0 && !into_counts;
  const CtkStructureView* into_view = into_counts ? &views[p.into] : nullptr;

  // 2. the origin
  if (p.origin_out != nullptr && blockIdx.x == 0 && tid == 0) {
    float o[12];
    ctk_structure_origin(p.origin_in != nullptr ? p.origin_in + g * 12 : nullptr, into_view, o);
    float* oo = p.origin_out + g * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) oo[i] = o[i];
  }
  if (n >= p.N_out) return;  // (no barrier follows)

  // 3. the slot
  const long gn = g * p.N + n;
  const bool has_first = p.first_row != nullptr;
  const int first = has_first ? p.first_row[gn] : 0;
  bool in_old = false, carried = false;
  float old[3] = {0.0f, 0.0f, 0.0f};
  if (p.structure_in != nullptr) {
    const float* sp = p.structure_in + gn * 3;
    const float s3[3] = {sp[0], sp[1], sp[2]};
    double Xo[3];
    in_old = ctk_structure_old(s3, p.valid_in[gn], has_first, first, p.source_frame, Xo);
    carried = in_old && !no_structure && ctk_structure_out(into_view, Xo, old);
  }
  const long row_n = g * p.R * (long)p.N + n;
  auto obs = [&](int j, int* qx, int* qy) {
    const int f = p.f0 + j;
    if (f < first) return false;
    const long at = row_n + (long)(f % p.R) * p.N;
    const float2 h = *reinterpret_cast<const float2*>(p.hc + at * 2);
    const bool okx = ctk_motion_quant(h.x, p.sx, qx), oky = ctk_motion_quant(h.y, p.sy, qy);
    if (!(okx && oky)) return false;
    return p.visible != nullptr ? p.visible[at] != 0 : ctk_draw_visible(p.hv[at], p.hf[at], p.thresh);
  };

  float point[3] = {0.0f, 0.0f, 0.0f}, err = -1.0f;
  int32_t st[4] = {0, 0, -1, 0};
  int lab;
  if (no_structure) {
    int m = 0;
    for (int j = 0; j < F; ++j) {
      int qx, qy;
      if (counts[j] != 0 && obs(j, &qx, &qy)) ++m;
    }
    st[0] = m, st[3] = CTK_STRUCTURE_BIT_INTO;
    lab = m >= 1 || in_old ? 0 : -1;
  } else if (carried && p.refine == 0) {
    point[0] = old[0], point[1] = old[1], point[2] = old[2];
    lab = 2;
  } else {
    lab = ctk_structure_slot(p.cam, views, counts, F, into_counts ? p.into : -1, p.tol, p.min_sin2, p.min_views, carried ? old : nullptr, obs,
                             point, &err, st);
  }
  const long o = g * p.N_out + n;
  float* po = p.points + o * 3;
  po[0] = point[0], po[1] = point[1], po[2] = point[2];
  p.label[o] = (int8_t)lab;
  p.error[o] = err;
  int32_t* so = p.stats + o * 4;
  so[0] = st[0], so[1] = st[1], so[2] = st[2], so[3] = st[3];
}

// everything but the pointers (whether `visible` is given is looked at)
int structure_check_shape(const ctk_fit_structure_args* a) {
  const long big = 1L << 30;
  if (a->G <= 0 || a->N <= 0 || a->N_out <= 0 || a->R <= 0 || a->N_out > a->N || a->N_out > CTK_STRUCTURE_POINTS_MAX) return CTK_E_SHAPE;
  if (a->F < 1 || a->F > CTK_STRUCTURE_VIEWS_MAX || a->F > a->R) return CTK_E_SHAPE;  // (rows of a ring must not alias)
  if (a->f0 < 0 || (long)a->f0 + a->F > big || a->G > 65535 || (long)a->G * a->N > (1L << 26) || (long)a->G * a->N * a->R > (1L << 40)) return CTK_E_SHAPE;
  if (a->into < -1 || a->into >= a->F) return CTK_E_SHAPE;
  if (a->source_frame < 0 || a->source_frame > big) return CTK_E_SHAPE;
  if (a->min_views < CTK_STRUCTURE_MIN_VIEWS || a->min_views > CTK_STRUCTURE_VIEWS_MAX) return CTK_E_SHAPE;
  if (a->refine < 0 || a->refine > 1) return CTK_E_SHAPE;
  if (!fit_scale_ok(a->tol)) return CTK_E_SHAPE;
  if (!(a->min_sin2 > 0.0f && a->min_sin2 <= 1.0f)) return CTK_E_SHAPE;
  if (!fit_scale_ok(a->fx) || !fit_scale_ok(a->fy) || !fit_finite(a->cx) || !fit_finite(a->cy)) return CTK_E_SHAPE;
  if (!fit_scale_ok(a->sx) || !fit_scale_ok(a->sy)) return CTK_E_SHAPE;
  if (a->visible == nullptr && a->thresh != a->thresh) return CTK_E_SHAPE;
  return CTK_OK;
}

}  // namespace

extern "C" int ctk_fit_structure_workspace_bytes(const ctk_fit_structure_args* a, size_t* out_bytes) {
  if (!a || !out_bytes) return CTK_E_NULL;
  const int rc = structure_check_shape(a);
  if (rc != CTK_OK) return rc;
  *out_bytes = 0;  // every slot is one thread's: nothing is shared beyond LDS
  return CTK_OK;
}

extern "C" int ctk_fit_structure(const ctk_fit_structure_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a) return CTK_E_NULL;
  if (!a->hist_coords || !a->pose || !a->points || !a->label || !a->error || !a->stats) return CTK_E_NULL;
  if (!a->visible && (!a->hist_vis || !a->hist_conf)) return CTK_E_NULL;
  if ((a->structure_in != nullptr) != (a->valid_in != nullptr)) return CTK_E_NULL;
  const int rc = structure_check_shape(a);
  if (rc != CTK_OK) return rc;
  (void)workspace, (void)workspace_bytes;  // the query answers 0: nothing is too small
  if ((reinterpret_cast<uintptr_t>(a->hist_coords) & 7u) != 0) return CTK_E_ALIGN;
  if (((reinterpret_cast<uintptr_t>(a->hist_vis) | reinterpret_cast<uintptr_t>(a->hist_conf) | reinterpret_cast<uintptr_t>(a->first_row) |
        reinterpret_cast<uintptr_t>(a->pose) | reinterpret_cast<uintptr_t>(a->pose_stats) | reinterpret_cast<uintptr_t>(a->structure_in) |
        reinterpret_cast<uintptr_t>(a->origin_in) | reinterpret_cast<uintptr_t>(a->points) | reinterpret_cast<uintptr_t>(a->error) |
        reinterpret_cast<uintptr_t>(a->stats) | reinterpret_cast<uintptr_t>(a->origin_out)) & 3u) != 0)
    return CTK_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);

  StructureParams p;
  p.G = a->G, p.N = a->N, p.N_out = a->N_out, p.R = a->R, p.f0 = a->f0, p.F = a->F, p.into = a->into, p.source_frame = a->source_frame;
  p.min_views = a->min_views, p.refine = a->refine;
  p.sx = a->sx, p.sy = a->sy, p.thresh = a->thresh, p.tol = a->tol, p.min_sin2 = a->min_sin2;
  p.cam.fx = (double)a->fx, p.cam.fy = (double)a->fy, p.cam.cx = (double)a->cx, p.cam.cy = (double)a->cy;
  p.hc = a->hist_coords, p.visible = a->visible, p.hv = a->hist_vis, p.hf = a->hist_conf, p.first_row = a->first_row;
  p.pose = a->pose, p.pose_stats = a->pose_stats, p.structure_in = a->structure_in, p.valid_in = a->valid_in, p.origin_in = a->origin_in;
  p.points = a->points, p.label = a->label, p.error = a->error, p.stats = a->stats, p.origin_out = a->origin_out;
  {
    CtkProfScope prof("fit_structure", 0.0, (double)a->G * a->N_out * (a->F * 5.0 * 120.0 + 100.0), s);
    const unsigned blocks = (unsigned)((a->N_out + ST_BLOCK - 1) / ST_BLOCK);
    hipLaunchKernelGGL(fit_structure_kernel, dim3(blocks, (unsigned)p.G), dim3(ST_BLOCK), 0, s, p);
  }
  CTK_HIP_CHECK_LAUNCH();
  return CTK_OK;
}
