"""ctypes binding of the C-ABI in include/ctk.h (libctk_hip.so, built by csrc/Makefile).

There is no CPU fallback: if the shared library is missing or cannot be loaded, importing any
op raises immediately.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CTK_LIB_PATH: dev knob for A/B runs of two builds in one GPU session (tools/gpu_session.sh); never set in product use
LIB_PATH = os.environ.get("CTK_LIB_PATH") or os.path.join(_HERE, "libctk_hip.so")

LEVELS = 4
DEPTH = 3
CORR_LD = 2432
CORR_K = 2401
X_LD = 1120
X_DIM = 1110
XF_LD = 1632     # CTK_XF_LD: the folded transformer input xf, 4 x 384 hidden columns + the 96 small-feature columns of x
XF_SMALL = 1536  # CTK_XF_SMALL: its first small-feature column (vis, conf, posenc 84, 10 zeros)
XF_DIM = 1622
HID = 384
MLP = 1536
VIRT = 64
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH = 0, 1, 2
ABI_VERSION = 9
MAX_BATCH = 16  # CTK_MAX_BATCH: videos of one joint window (ctk_forward_window_batch)
STREAM_EMPTY_FRAME = float(2 ** 30)  # CTK_STREAM_EMPTY_FRAME: the query frame of an empty slot of a stream (ctk_stream_assign)
# ctk_window_batch.flags: the B windows are B query groups of ONE video -- the same fmaps pointers in every group, and coords / vis /
# conf / support[l] / point_mask of group b lying right behind group b - 1 in one allocation each (include/ctk.h).  The library
# then keeps ONE split-half pyramid copy and launches the correlation sampler once per chunk piece over all groups.
BATCH_SHARED_FMAPS = 1
INGEST_U8, INGEST_F32 = 0, 1  # ctk_ingest_args.dtype
INGEST_HWC, INGEST_CHW = 0, 1  # ctk_ingest_args.layout
PAD_ZEROS, PAD_BORDER = 0, 1  # ctk_bilinear_sampler padding_mode
# ctk_set_option keys (include/ctk.h)
(OPT_GEMM_PP, OPT_GEMM_TAIL_PCT, OPT_CORR_VERSION, OPT_CORR_MAP, OPT_ATTENTION_VALU, OPT_ATTENTION_TIME_PERSISTENT,
 OPT_OVERLAP) = range(7)
OPT_COUNT = 7
LENS_TO_IDEAL, LENS_TO_SENSOR = 0, 1  # ctk_lens_*_args.direction
LENS_ROUNDS = 8  # CTK_LENS_ROUNDS: Newton rounds of the inverse (csrc/lens_math.h)

_fp = C.c_void_p  # device pointers travel as integers


class BlockWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("wq", "bq", "wkv", "bkv", "wo", "bo", "w1", "b1", "w2", "b2", "ctx_gamma", "ctx_beta",
                                   "wq_p", "wkv_p", "wo_p", "w1_p", "w2_p")]


class ModelWeights(C.Structure):
    _fields_ = [(n, _fp) for n in ("corr_fc1_w", "corr_fc1_b", "corr_fc2_w", "corr_fc2_b", "in_w", "in_bias_t",
                                   "virtual_tokens", "head_w", "head_b", "corr_fc1_p", "corr_fc2_p", "in_p")] + [
        ("time_blocks", BlockWeights * DEPTH),
        ("virtual2point", BlockWeights * DEPTH),
        ("virtual_self", BlockWeights * DEPTH),
        ("point2virtual", BlockWeights * DEPTH),
    ]


WINDOW_NO_SPACE_ATTN = 1  # ctk_window_args.flags


class WindowArgs(C.Structure):
    _fields_ = [
        ("S", C.c_int32), ("N", C.c_int32), ("iters", C.c_int32),
        ("H", C.c_int32 * LEVELS), ("W", C.c_int32 * LEVELS),
        ("fmaps", _fp * LEVELS), ("support", _fp * LEVELS),
        ("point_mask", _fp),
        ("coords", _fp), ("vis", _fp), ("conf", _fp),
        ("scale_x", C.c_float), ("scale_y", C.c_float),
        ("points_per_chunk", C.c_int32),
        ("aux_stream", _fp),
        ("flags", C.c_int32),
    ]


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", _fp), ("lda", C.c_int64), ("M", C.c_int32),
        ("W", _fp), ("ldw", C.c_int64), ("N", C.c_int32), ("K", C.c_int32),
        ("Wp", _fp),
        ("C", _fp), ("ldc", C.c_int64),
        ("bias", _fp),
        ("bias_rows", _fp), ("bias_period", C.c_int32),
        ("resid", _fp), ("ldr", C.c_int64),
        ("act", C.c_int32),
        ("batch", C.c_int32), ("a_bs", C.c_int64), ("c_bs", C.c_int64),
        ("k_valid", C.c_int32), ("a_split", C.c_int32), ("c_split", C.c_int32),
    ]


class AttnArgs(C.Structure):
    _fields_ = [
        ("q", _fp), ("q_ld", C.c_int64), ("q_bs", C.c_int64), ("q_is", C.c_int64),
        ("k", _fp), ("v", _fp), ("kv_ld", C.c_int64), ("kv_bs", C.c_int64), ("kv_is", C.c_int64),
        ("out", _fp), ("o_ld", C.c_int64), ("o_bs", C.c_int64), ("o_is", C.c_int64),
        ("nbatch", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32),
        ("splits", C.c_int32), ("partial", _fp), ("o_split", C.c_int32),
        ("key_mask", _fp), ("query_mask", _fp),
    ]


class AttnBatch2(C.Structure):
    """ctk_attn_batch2: the two-level batch of ctk_attention_ex (outer strides in rows / mask bytes)."""
    _fields_ = [("inner", C.c_int32), ("reserved", C.c_int32), ("q_os", C.c_int64), ("kv_os", C.c_int64), ("o_os", C.c_int64),
                ("key_mask_os", C.c_int64), ("query_mask_os", C.c_int64)]


class WindowBatch(C.Structure):
    """ctk_window_batch: B windows of equal shape for one joint call; flags = 0 or BATCH_SHARED_FMAPS."""
    _fields_ = [("B", C.c_int32), ("flags", C.c_int32), ("videos", C.POINTER(WindowArgs))]


class StreamArgs(C.Structure):
    """ctk_stream_args: the device-resident stream state of G query groups over one live video (include/ctk.h)."""
    _fields_ = [
        ("G", C.c_int32), ("N", C.c_int32), ("S", C.c_int32), ("step", C.c_int32),
        ("ind", C.c_int32), ("T_valid", C.c_int32), ("T_cap", C.c_int32), ("stride", C.c_float),
        ("queries", _fp), ("hist_coords", _fp), ("hist_vis", _fp), ("hist_conf", _fp),
        ("coords", _fp), ("vis", _fp), ("conf", _fp), ("point_mask", _fp),
        ("H", C.c_int32 * LEVELS), ("W", C.c_int32 * LEVELS),
        ("fmaps", _fp * LEVELS), ("support", _fp * LEVELS),
        ("nonfinite", _fp),
    ]


class StreamEmit:
    """Holder of ctk_stream_emit_args (include/ctk.h, "endless streams").  The mirror is the nested class: the module-level
    Structure classes are the census of tests/ctk_support.py::abi_structs(), which this additive struct does not join; its layout
    is checked against the compiler by tests/test_stream_ring_cabi.py."""

    class Args(C.Structure):
        """ctk_stream_emit_args: history frames [f0, f1) -> contiguous tracks, logits, visibility."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("f1", C.c_int32),
            ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float), ("reserved", C.c_int32),
            ("hist_coords", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("tracks", _fp), ("vis_logit", _fp), ("conf_logit", _fp), ("visible", _fp),
        ]


class StreamHealth:
    """Holder of ctk_stream_health_args (include/ctk.h, "health"), nested like StreamEmit.Args and for the same reason; its layout is
    checked against the compiler by tests/test_stream_health_cabi.py."""

    class Args(C.Structure):
        """ctk_stream_health_args: the last `look` frames of every slot -> frames lost, coverage cell, points per cell."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f1", C.c_int32), ("look", C.c_int32),
            ("ind_next", C.c_int32), ("thresh", C.c_float),
            ("x_lo", C.c_float), ("x_hi", C.c_float), ("y_lo", C.c_float), ("y_hi", C.c_float),
            ("gh", C.c_int32), ("gw", C.c_int32), ("inv_cw", C.c_float), ("inv_ch", C.c_float), ("reserved", C.c_int32),
            ("queries", _fp), ("hist_coords", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("lost", _fp), ("cell", _fp), ("cover", _fp),
        ]


class Seed:
    """Holder of ctk_seed_args (include/ctk.h, "seed points"), nested like StreamEmit.Args and for the same reason; its layout is checked
    against the compiler by tests/test_stream_seed_cabi.py."""

    class Args(C.Structure):
        """ctk_seed_args: one frame and a grid of cells -> the best-textured pixel of every cell."""
        _fields_ = [
            ("frame", _fp), ("h", C.c_int32), ("w", C.c_int32),
            ("radius", C.c_int32), ("margin", C.c_int32), ("inset", C.c_int32), ("min_score", C.c_int32),
            ("x_lo", C.c_float), ("x_hi", C.c_float), ("y_lo", C.c_float), ("y_hi", C.c_float),
            ("gh", C.c_int32), ("gw", C.c_int32), ("inv_cw", C.c_float), ("inv_ch", C.c_float), ("reserved", C.c_int32),
            ("seeds", _fp),
        ]


class Draw:
    """Holder of ctk_draw_args (include/ctk.h, "draw tracks"), nested like StreamEmit.Args and for the same reason; its layout is checked
    against the compiler by tests/test_draw_cabi.py."""

    TRAIL_MAX, RADIUS_MAX, HALF_WIDTH_MAX, JUMP_MAX = 64, 32, 16, 4095

    class Args(C.Structure):
        """ctk_draw_args: history rows, colours and uint8 frames -> marks and trails drawn onto the frames."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("trail", C.c_int32), ("radius", C.c_int32), ("half_width", C.c_int32), ("max_jump", C.c_int32),
            ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float), ("layout", C.c_int32),
            ("H", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_uint8 * 65),
            ("frame_stride", C.c_int64), ("row_stride", C.c_int64),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp), ("colors", _fp),
            ("src", _fp), ("dst", _fp),
        ]


class Motion:
    """Holder of ctk_fit_motion_args (include/ctk.h, "fit motion"), nested like StreamEmit.Args and for the same reason; its layout is
    checked against the compiler by tests/test_motion_cabi.py."""

    TRANSLATION, SIMILARITY = 0, 1
    POINTS_MAX, HYPOTHESES_MAX = 8192, 4096

    class Args(C.Structure):
        """ctk_fit_motion_args: history rows -> per frame a 2 x 3 motion matrix, an inlier mark per point and the fit's counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("lag", C.c_int32), ("model", C.c_int32), ("K", C.c_int32), ("seed", C.c_uint32),
            ("tol", C.c_float), ("min_base", C.c_float), ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("motion", _fp), ("inlier", _fp), ("stats", _fp),
        ]


class Warp:
    """Holder of ctk_warp_args and ctk_smooth_path_args (include/ctk.h, "warp frames"), nested like Motion.Args and for the same reason;
    their layouts are checked against the compiler by tests/test_warp_cabi.py."""

    BORDER_FILL, BORDER_EDGE = 0, 1

    class Args(C.Structure):
        """ctk_warp_args: uint8 pictures and one 2 x 3 matrix each -> the resampled pictures."""
        _fields_ = [
            ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("layout", C.c_int32), ("border", C.c_int32), ("reserved", C.c_int32),
            ("fill", C.c_uint8 * 4),
            ("src_frame_stride", C.c_int64), ("src_row_stride", C.c_int64), ("dst_frame_stride", C.c_int64), ("dst_row_stride", C.c_int64),
            ("matrices", _fp), ("src", _fp), ("dst", _fp),
        ]

    class PathArgs(C.Structure):
        """ctk_smooth_path_args: per-frame camera motions and a persistent state -> the warp matrices that steady the camera."""
        _fields_ = [
            ("G", C.c_int32), ("F", C.c_int32), ("alpha", C.c_float), ("reserved", C.c_int32),
            ("motion", _fp), ("post", _fp), ("state", _fp), ("warp", _fp),
        ]


class Lens:
    """Holder of ctk_lens, ctk_lens_frames_args and ctk_lens_points_args (include/ctk.h, "lens"), nested like Warp.Args and for the same
    reason; their layouts are checked against the compiler by tests/test_lens_cabi.py.  The bounds mirror csrc/lens_math.h."""

    FOCAL_MIN, FOCAL_MAX, REACH, COEFF_MAX, POINTS_MAX = 1.0, 1e6, 32768.0, 64.0, 1 << 20

    class Camera(C.Structure):
        """ctk_lens: sensor and ideal intrinsics (fx, fy, cx, cy) and the five Brown-Conrady coefficients (k1, k2, p1, p2, k3)."""
        _fields_ = [("sensor", C.c_double * 4), ("ideal", C.c_double * 4), ("k", C.c_double * 5), ("reserved", C.c_double)]

    class FramesArgs(C.Structure):
        """ctk_lens_frames_args: uint8 pictures on sensor pixels -> the pinhole pictures, or back; of a size of their own."""

    class PointsArgs(C.Structure):
        """ctk_lens_points_args: positions [G,F,N,2] in sensor pixels -> ideal pixels, or back, and a label per point."""


# (a nested class body does not see its neighbour Camera: the two structs that embed it get their fields here)
Lens.FramesArgs._fields_ = [
    ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("layout", C.c_int32),
    ("border", C.c_int32), ("direction", C.c_int32), ("tol", C.c_float), ("reserved", C.c_int32), ("fill", C.c_uint8 * 4),
    ("src_frame_stride", C.c_int64), ("src_row_stride", C.c_int64), ("dst_frame_stride", C.c_int64), ("dst_row_stride", C.c_int64),
    ("lens", Lens.Camera), ("src", _fp), ("dst", _fp),
]
Lens.PointsArgs._fields_ = [
    ("G", C.c_int32), ("F", C.c_int32), ("N", C.c_int32), ("direction", C.c_int32), ("tol", C.c_float), ("reserved", C.c_int32),
    ("src_group_stride", C.c_int64), ("src_frame_stride", C.c_int64), ("dst_group_stride", C.c_int64), ("dst_frame_stride", C.c_int64),
    ("lens", Lens.Camera), ("src", _fp), ("dst", _fp), ("label", _fp),
]


class Field:
    """Holder of ctk_track_field_args and ctk_warp_field_args (include/ctk.h, "track field"), nested like Warp.Args and for the same
    reason; their layouts are checked against the compiler by tests/test_field_cabi.py."""

    POINTS_MAX, CS_MIN, CS_MAX, RADIUS_MAX, NO_LEVEL = 8192, 2, 6, 4, 255

    class Args(C.Structure):
        """ctk_track_field_args: history rows -> per frame a grid of displacements towards another frame, their levels and the counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("H", C.c_int32), ("W", C.c_int32), ("cs", C.c_int32), ("radius", C.c_int32), ("to", C.c_int32), ("lag", C.c_int32),
            ("anchor_frame", C.c_int32), ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float), ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp),
            ("field", _fp), ("level", _fp), ("stats", _fp),
        ]

    class WarpArgs(C.Structure):
        """ctk_warp_field_args: uint8 pictures and one field each -> the pictures resampled through it, and the dense flow."""
        _fields_ = [
            ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("layout", C.c_int32), ("border", C.c_int32),
            ("cs", C.c_int32), ("reserved", C.c_int32), ("fill", C.c_uint8 * 4),
            ("src_frame_stride", C.c_int64), ("src_row_stride", C.c_int64), ("dst_frame_stride", C.c_int64), ("dst_row_stride", C.c_int64),
            ("field", _fp), ("src", _fp), ("dst", _fp), ("flow", _fp),
        ]


class Objects:
    """Holder of ctk_fit_objects_args (include/ctk.h, "fit objects"), nested like Motion.Args and for the same reason; its layout is
    checked against the compiler by tests/test_objects_cabi.py."""

    OBJECTS_MAX, NONE = 16, 127

    class Args(C.Structure):
        """ctk_fit_objects_args: history rows (and labels, or none) -> per frame up to L motion matrices, a label per point, and each
        fit's counts and box."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("L", C.c_int32), ("min_points", C.c_int32),
            ("model", C.c_int32), ("K", C.c_int32), ("seed", C.c_uint32),
            ("tol", C.c_float), ("min_base", C.c_float), ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp), ("labels", _fp),
            ("motion", _fp), ("label", _fp), ("stats", _fp), ("box", _fp),
        ]


class Planes:
    """Holder of ctk_fit_planes_args and ctk_warp_planes_args (include/ctk.h, "fit planes / warp planes"), nested like Objects.Args and
    for the same reason; their layouts are checked against the compiler by tests/test_planes_cabi.py.  The constants mirror
    csrc/plane_math.h."""

    PLANES_MAX, NONE, BORDER_KEEP = 16, 127, 2

    class Args(C.Structure):
        """ctk_fit_planes_args: history rows (and labels, or none) -> per frame up to L homographies, a label per point, and each
        fit's counts and box."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("L", C.c_int32), ("min_points", C.c_int32),
            ("inverse", C.c_int32), ("K", C.c_int32), ("seed", C.c_uint32),
            ("tol", C.c_float), ("min_base", C.c_float), ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp), ("labels", _fp),
            ("homography", _fp), ("label", _fp), ("stats", _fp), ("box", _fp),
        ]

    class WarpArgs(C.Structure):
        """ctk_warp_planes_args: uint8 pictures and one 3 x 3 matrix each -> the resampled pictures, of a size of their own."""
        _fields_ = [
            ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("C", C.c_int32),
            ("layout", C.c_int32), ("border", C.c_int32), ("reserved", C.c_int32), ("fill", C.c_uint8 * 4),
            ("src_frame_stride", C.c_int64), ("src_row_stride", C.c_int64), ("dst_frame_stride", C.c_int64), ("dst_row_stride", C.c_int64),
            ("matrices", _fp), ("src", _fp), ("dst", _fp),
        ]


class Epipolar:
    """Holder of ctk_fit_epipolar_args (include/ctk.h, "fit epipolar"), nested like Planes.Args and for the same reason; its layout is
    checked against the compiler by tests/test_epipolar_cabi.py.  The constants mirror csrc/epipolar_math.h."""

    SAMPLE, MIN_POINTS = 8, 8

    class Args(C.Structure):
        """ctk_fit_epipolar_args: history rows (and a mask, or none) -> per frame one fundamental matrix, a label and a squared Sampson
        distance per point, and the fit's counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("min_points", C.c_int32), ("K", C.c_int32),
            ("seed", C.c_uint32),
            ("tol", C.c_float), ("min_base", C.c_float), ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp), ("mask", _fp),
            ("fundamental", _fp), ("label", _fp), ("error", _fp), ("stats", _fp),
        ]


class Pose:
    """Holder of ctk_fit_pose_args (include/ctk.h, "fit pose"), nested like Epipolar.Args and for the same reason; its layout is checked
    against the compiler by tests/test_pose_cabi.py.  The constants mirror csrc/pose_math.h."""

    MIN_POINTS, SUMS, ROUNDS = 8, 28, 2

    class Args(C.Structure):
        """ctk_fit_pose_args: history rows, four intrinsics and what ctk_fit_epipolar wrote (fundamental, label) -> per frame a pose
        (R | t), two depths per point, and the fit's counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("min_points", C.c_int32),
            ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
            ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp), ("mask", _fp),
            ("fundamental", _fp), ("label", _fp), ("pose", _fp), ("depth", _fp), ("stats", _fp),
        ]


class Resection:
    """Holder of ctk_fit_resection_args (include/ctk.h, "fit resection"), nested like Pose.Args and for the same reason; its layout is
    checked against the compiler by tests/test_resection_cabi.py.  The constants mirror csrc/resection_math.h."""

    LIST_MAX, MIN_POINTS, HYPOTHESES_MAX, ROUNDS = 4096, 6, 1024, 3

    class Args(C.Structure):
        """ctk_fit_resection_args: history rows, four intrinsics, a 3-D structure and a seed pose per frame -> per frame a pose (R | t)
        in the structure's unit, a label and a reprojection error per point, and the fit's counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("min_points", C.c_int32),
            ("hypotheses", C.c_int32), ("seed", C.c_uint32),
            ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
            ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float), ("tol", C.c_float),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp),
            ("structure", _fp), ("valid", _fp), ("seed_pose", _fp), ("pose", _fp), ("label", _fp), ("error", _fp), ("stats", _fp),
        ]


class P3p:
    """Holder of ctk_fit_p3p_args (include/ctk.h, "fit p3p"), nested like Resection.Args and for the same reason; its layout is checked
    against the compiler by tests/test_p3p_cabi.py.  The constants mirror csrc/p3p_math.h; the list cap, min_points and the ceiling of
    `hypotheses` are Resection's."""

    ROUNDS = 6

    class Args(C.Structure):
        """ctk_fit_p3p_args: ctk_fit_resection_args without seed_pose -> per frame a pose (R | t) in the structure's unit, a label and
        a reprojection error per point, and the fit's counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("min_points", C.c_int32),
            ("hypotheses", C.c_int32), ("seed", C.c_uint32),
            ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
            ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float), ("tol", C.c_float),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp),
            ("structure", _fp), ("valid", _fp), ("pose", _fp), ("label", _fp), ("error", _fp), ("stats", _fp),
        ]


class Focal:
    """Holder of ctk_fit_focal_args (include/ctk.h, "fit focal"), nested like Pose.Args and for the same reason; its layout is checked
    against the compiler by tests/test_focal_cabi.py.  The constants mirror csrc/focal_math.h; min_points is Pose's."""

    K_MAX, FRAMES_MAX, ONE = 256, 65535, 1 << 32
    BIT_END, BIT_FLAT, BIT_CANDIDATE = 1, 2, 4

    class Args(C.Structure):
        """ctk_fit_focal_args: history rows, a principal point, what ctk_fit_epipolar wrote (fundamental, label) and K candidate focal
        lengths -> per (frame, candidate) an integer cost, per group the summed curve, the chosen focal length and the counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("to", C.c_int32), ("lag", C.c_int32), ("anchor_frame", C.c_int32), ("min_points", C.c_int32),
            ("K", C.c_int32), ("min_frames", C.c_int32),
            ("cx", C.c_float), ("cy", C.c_float), ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float),
            ("tol", C.c_float), ("contrast", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("anchor_coords", _fp), ("anchor_visible", _fp), ("mask", _fp),
            ("fundamental", _fp), ("label", _fp), ("focals", _fp), ("curve_in", _fp),
            ("focal", _fp), ("curve", _fp), ("cost", _fp), ("stats", _fp),
        ]


class Align:
    """Holder of ctk_fit_align_args (include/ctk.h, "fit align"), nested like Resection.Args and for the same reason; its layout is
    checked against the compiler by tests/test_align_cabi.py.  The constants mirror csrc/align_math.h; the list cap and the ceiling of
    `hypotheses` are Resection's."""

    MIN_POINTS, ROUNDS, REACH = 3, 3, 1048576.0
    BIT_ROUND, BIT_LEFT, BIT_CAP, BIT_IDENTICAL = 2, 4, 8, 32

    class Args(C.Structure):
        """ctk_fit_align_args: two point sets with their validity bytes, a camera for the second, two tolerances -> per pair the
        similarity (s R | t) and its scale, a label and a squared pixel distance per slot, and the fit's counts."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("min_points", C.c_int32), ("hypotheses", C.c_int32), ("seed", C.c_uint32),
            ("reserved", C.c_int32),
            ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("tol", C.c_float), ("depth_tol", C.c_float),
            ("a", _fp), ("valid_a", _fp), ("b", _fp), ("valid_b", _fp), ("mask", _fp),
            ("sim", _fp), ("scale", _fp), ("label", _fp), ("error", _fp), ("stats", _fp),
        ]


class Structure3D:
    """Holder of ctk_fit_structure_args (include/ctk.h, "fit structure"), nested like Resection.Args and for the same reason; its layout
    is checked against the compiler by tests/test_structure_cabi.py.  The constants mirror csrc/structure_math.h."""

    VIEWS_MAX, POINTS_MAX, MIN_VIEWS, ROUNDS = 256, 8192, 2, 3
    BIT_ROUND1, BIT_ROUND2, BIT_ROUND3, BIT_NO_START, BIT_NO_PARALLAX, BIT_INTO, BIT_MINORITY = 1, 2, 4, 8, 16, 32, 64

    class Args(C.Structure):
        """ctk_fit_structure_args: history rows, four intrinsics, a pose per view, optionally the old structure and its origin -> per
        slot a 3-D point, a label, a mean reprojection error and the counts; per group the new origin."""
        _fields_ = [
            ("G", C.c_int32), ("N", C.c_int32), ("N_out", C.c_int32), ("R", C.c_int32), ("f0", C.c_int32), ("F", C.c_int32),
            ("into", C.c_int32), ("source_frame", C.c_int32), ("min_views", C.c_int32), ("refine", C.c_int32),
            ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
            ("sx", C.c_float), ("sy", C.c_float), ("thresh", C.c_float), ("tol", C.c_float), ("min_sin2", C.c_float),
            ("reserved", C.c_int32),
            ("hist_coords", _fp), ("visible", _fp), ("hist_vis", _fp), ("hist_conf", _fp), ("first_row", _fp),
            ("pose", _fp), ("pose_stats", _fp), ("structure_in", _fp), ("valid_in", _fp), ("origin_in", _fp),
            ("points", _fp), ("label", _fp), ("error", _fp), ("stats", _fp), ("origin_out", _fp),
        ]


class IngestArgs(C.Structure):
    """ctk_ingest_args: raw frames -> the encoder's planar float32 input (include/ctk.h, "frame ingest")."""
    _fields_ = [
        ("src", _fp), ("dtype", C.c_int32), ("layout", C.c_int32),
        ("F", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("reserved", C.c_int32),
        ("frame_stride", C.c_int64), ("row_stride", C.c_int64),
        ("dst", _fp),
    ]


class FormerWeights(C.Structure):
    """ctk_former_weights: the general update former (CoTracker2)."""
    _fields_ = [
        ("depth", C.c_int32), ("in_dim", C.c_int32), ("in_ld", C.c_int32), ("out_dim", C.c_int32), ("out_ld", C.c_int32),
        ("in_w", _fp), ("in_p", _fp), ("in_b", _fp), ("in_bias_t", _fp), ("virtual_tokens", _fp),
        ("head_w", _fp), ("head_p", _fp), ("head_b", _fp),
        ("time_blocks", C.POINTER(BlockWeights)), ("virtual2point", C.POINTER(BlockWeights)),
        ("virtual_self", C.POINTER(BlockWeights)), ("point2virtual", C.POINTER(BlockWeights)),
    ]


class V2WindowArgs(C.Structure):
    """ctk_v2_window_args: one CoTracker2 window (cotracker.py:86-173)."""
    _fields_ = [
        ("S", C.c_int32), ("N", C.c_int32), ("iters", C.c_int32),
        ("H", C.c_int32 * LEVELS), ("W", C.c_int32 * LEVELS),
        ("fmaps", _fp * LEVELS),
        ("coords", _fp), ("track_feat", _fp), ("vis", _fp), ("track_mask", _fp), ("point_mask", _fp), ("vis_out", _fp),
    ]


class V2Weights(C.Structure):
    """ctk_v2_weights."""
    _fields_ = [
        ("former", FormerWeights),
        ("pos_hwc", _fp), ("pos_h", C.c_int32), ("pos_w", C.c_int32),
        ("norm_w", _fp), ("norm_b", _fp),
        ("upd_w", _fp), ("upd_p", _fp), ("upd_b", _fp),
        ("vis_w", _fp), ("vis_b", _fp),
    ]


class ProfileRow(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


# every symbol include/ctk.h declares: (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "ctk_abi_version": (C.c_int, []),
    "ctk_error_string": (C.c_char_p, [C.c_int]),
    "ctk_forward_window_workspace_bytes": (C.c_int, [_P(WindowArgs), _P(C.c_size_t)]),
    "ctk_forward_window": (C.c_int, [_P(WindowArgs), _P(ModelWeights), _fp, C.c_size_t, _fp]),
    "ctk_window_graph_create": (C.c_int, [_P(WindowArgs), _P(ModelWeights), _fp, C.c_size_t, _P(C.c_void_p)]),
    "ctk_forward_window_batch_workspace_bytes": (C.c_int, [_P(WindowBatch), _P(C.c_size_t)]),
    "ctk_forward_window_batch": (C.c_int, [_P(WindowBatch), _P(ModelWeights), _fp, C.c_size_t, _fp]),
    "ctk_window_batch_graph_create": (C.c_int, [_P(WindowBatch), _P(ModelWeights), _fp, C.c_size_t, _P(C.c_void_p)]),
    "ctk_corr_embed_batch_workspace_bytes": (C.c_int, [_P(WindowBatch), _P(C.c_size_t)]),
    "ctk_corr_embed_batch": (C.c_int, [_P(WindowBatch), _P(ModelWeights), _fp, _fp, C.c_size_t, _fp]),
    "ctk_window_tokens_batch": (C.c_int, [_P(WindowBatch), _P(ModelWeights), _fp, _fp, C.c_size_t, _fp]),
    "ctk_window_graph_launch": (C.c_int, [C.c_void_p, _fp]),
    "ctk_window_graph_nodes": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "ctk_window_graph_destroy": (C.c_int, [C.c_void_p]),
    "ctk_stream_begin": (C.c_int, [_P(StreamArgs), _fp]),
    "ctk_stream_support": (C.c_int, [_P(StreamArgs), _fp]),
    "ctk_stream_commit": (C.c_int, [_P(StreamArgs), _fp]),
    "ctk_stream_assign": (C.c_int, [_P(StreamArgs), _fp, _fp, C.c_int32, C.c_int32, _fp]),
    "ctk_stream_begin_ring": (C.c_int, [_P(StreamArgs), _fp]),
    "ctk_stream_support_ring": (C.c_int, [_P(StreamArgs), _fp]),
    "ctk_stream_commit_ring": (C.c_int, [_P(StreamArgs), _fp]),
    "ctk_stream_assign_ring": (C.c_int, [_P(StreamArgs), _fp, _fp, C.c_int32, _fp]),
    "ctk_stream_assign_resident": (C.c_int, [_P(StreamArgs), _fp, _fp, C.c_int32, C.c_int32, _fp]),
    "ctk_stream_assign_resident_ring": (C.c_int, [_P(StreamArgs), _fp, _fp, C.c_int32, _fp]),
    "ctk_stream_emit": (C.c_int, [_P(StreamEmit.Args), _fp]),
    "ctk_stream_health": (C.c_int, [_P(StreamHealth.Args), _fp]),
    "ctk_seed_points": (C.c_int, [_P(Seed.Args), _fp]),
    "ctk_ingest_frames": (C.c_int, [_P(IngestArgs), _fp]),
    "ctk_draw_tracks_workspace_bytes": (C.c_int, [_P(Draw.Args), _P(C.c_size_t)]),
    "ctk_draw_tracks": (C.c_int, [_P(Draw.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_motion_workspace_bytes": (C.c_int, [_P(Motion.Args), _P(C.c_size_t)]),
    "ctk_fit_motion": (C.c_int, [_P(Motion.Args), _fp, C.c_size_t, _fp]),
    "ctk_warp_frames": (C.c_int, [_P(Warp.Args), _fp]),
    "ctk_smooth_path": (C.c_int, [_P(Warp.PathArgs), _fp]),
    "ctk_lens_frames": (C.c_int, [_P(Lens.FramesArgs), _fp]),
    "ctk_lens_points": (C.c_int, [_P(Lens.PointsArgs), _fp]),
    "ctk_track_field_workspace_bytes": (C.c_int, [_P(Field.Args), _P(C.c_size_t)]),
    "ctk_track_field": (C.c_int, [_P(Field.Args), _fp, C.c_size_t, _fp]),
    "ctk_warp_field": (C.c_int, [_P(Field.WarpArgs), _fp]),
    "ctk_fit_objects_workspace_bytes": (C.c_int, [_P(Objects.Args), _P(C.c_size_t)]),
    "ctk_fit_objects": (C.c_int, [_P(Objects.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_planes_workspace_bytes": (C.c_int, [_P(Planes.Args), _P(C.c_size_t)]),
    "ctk_fit_planes": (C.c_int, [_P(Planes.Args), _fp, C.c_size_t, _fp]),
    "ctk_warp_planes": (C.c_int, [_P(Planes.WarpArgs), _fp]),
    "ctk_fit_epipolar_workspace_bytes": (C.c_int, [_P(Epipolar.Args), _P(C.c_size_t)]),
    "ctk_fit_epipolar": (C.c_int, [_P(Epipolar.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_pose_workspace_bytes": (C.c_int, [_P(Pose.Args), _P(C.c_size_t)]),
    "ctk_fit_pose": (C.c_int, [_P(Pose.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_resection_workspace_bytes": (C.c_int, [_P(Resection.Args), _P(C.c_size_t)]),
    "ctk_fit_resection": (C.c_int, [_P(Resection.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_p3p_workspace_bytes": (C.c_int, [_P(P3p.Args), _P(C.c_size_t)]),
    "ctk_fit_p3p": (C.c_int, [_P(P3p.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_align_workspace_bytes": (C.c_int, [_P(Align.Args), _P(C.c_size_t)]),
    "ctk_fit_align": (C.c_int, [_P(Align.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_focal_workspace_bytes": (C.c_int, [_P(Focal.Args), _P(C.c_size_t)]),
    "ctk_fit_focal": (C.c_int, [_P(Focal.Args), _fp, C.c_size_t, _fp]),
    "ctk_fit_structure_workspace_bytes": (C.c_int, [_P(Structure3D.Args), _P(C.c_size_t)]),
    "ctk_fit_structure": (C.c_int, [_P(Structure3D.Args), _fp, C.c_size_t, _fp]),
    "ctk_corr_embed_workspace_bytes": (C.c_int, [_P(WindowArgs), _P(C.c_size_t)]),
    "ctk_corr_embed": (C.c_int, [_P(WindowArgs), _P(ModelWeights), _fp, _fp, C.c_size_t, _fp]),
    "ctk_corr_volume": (C.c_int, [_P(WindowArgs), _fp, _fp]),
    "ctk_corr_volume_sh_workspace_bytes": (C.c_int, [_P(WindowArgs), _P(C.c_size_t)]),
    "ctk_corr_volume_sh": (C.c_int, [_P(WindowArgs), _fp, _fp, C.c_size_t, _fp]),
    "ctk_assemble_tokens": (C.c_int, [_P(WindowArgs), _fp, C.c_int32, _fp]),
    "ctk_assemble_tokens_batch": (C.c_int, [_P(WindowBatch), _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "ctk_virtual_init": (C.c_int, [_fp, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_heads_update": (C.c_int, [_P(WindowBatch), _fp, _fp, _fp, _fp, _fp]),
    "ctk_update_former_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, _P(C.c_size_t)]),
    "ctk_update_former": (C.c_int, [C.c_int32, C.c_int32, _fp, _P(ModelWeights), _fp, _fp, C.c_size_t, _fp]),
    "ctk_update_former_ex": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_int32, _P(FormerWeights), _fp, _fp, _fp, C.c_size_t, _fp]),
    "ctk_forward_window_v2_workspace_bytes": (C.c_int, [_P(V2WindowArgs), _P(V2Weights), _P(C.c_size_t)]),
    "ctk_forward_window_v2": (C.c_int, [_P(V2WindowArgs), _P(V2Weights), _fp, C.c_size_t, _fp]),
    "ctk_v2_window_graph_create": (C.c_int, [_P(V2WindowArgs), _P(V2Weights), _fp, C.c_size_t, _P(C.c_void_p)]),
    "ctk_v2_assemble": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int32, _fp, C.c_int32, _fp]),
    "ctk_v2_apply_delta": (C.c_int, [C.c_int32, C.c_int32, _fp, C.c_int32, _fp, _fp, _fp, C.c_float, _fp, _fp]),
    "ctk_v2_vis_head": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, _fp]),
    "ctk_sample_features4d": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, _fp, _fp]),
    "ctk_bilinear_sampler": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int64, C.c_int32,
                                       C.c_int32, _fp, _fp]),
    "ctk_tap_indices": (C.c_int, [_P(WindowArgs), _fp, _fp]),
    "ctk_sample_patches": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_sample_support": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp]),
    "ctk_corrblock_sample": (C.c_int, [_P(_fp), _P(C.c_int32), _P(C.c_int32), C.c_int32, C.c_int32, _fp, _fp, _fp, _fp]),
    "ctk_normalize_to_nhwc": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_avg_pool2_nhwc": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_conv2d_sh": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, _fp, _fp, _fp]),
    "ctk_enc_stem_im2col": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_enc_inorm_workspace_bytes": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, _P(C.c_size_t)]),
    "ctk_enc_inorm_stats": (C.c_int, [_fp, C.c_int32, C.c_int64, C.c_int32, C.c_float, _fp, _fp, _fp]),
    "ctk_enc_inorm_apply": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int32, C.c_int64, C.c_int32, _fp, _fp, _fp]),
    "ctk_enc_fuse": (C.c_int, [_P(_fp), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), C.c_int32, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_enc_l2norm": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "ctk_gemm": (C.c_int, [_P(GemmArgs), _fp]),
    "ctk_pack_weight_bytes": (C.c_int, [C.c_int32, C.c_int32, _P(C.c_size_t)]),
    "ctk_pack_weight": (C.c_int, [_fp, C.c_int64, C.c_int32, C.c_int32, _fp, _fp]),
    "ctk_layernorm": (C.c_int, [_fp, _fp, C.c_int64, _fp, _fp, C.c_float, C.c_int32, _fp]),
    "ctk_layernorm_dual": (C.c_int, [_fp, _fp, _fp, C.c_int64, _fp, _fp, C.c_float, C.c_float, C.c_int32, _fp]),
    "ctk_split_rows": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, _fp, _fp]),
    "ctk_attention": (C.c_int, [_P(AttnArgs), _fp]),
    "ctk_attention_ex": (C.c_int, [_P(AttnArgs), _P(AttnBatch2), _fp]),
    "ctk_profile_enable": (C.c_int, [C.c_int]),
    "ctk_gemm_pp_mode": (None, [C.c_int]),
    "ctk_set_option": (C.c_int, [C.c_int, C.c_int]),
    "ctk_get_option": (C.c_int, [C.c_int, _P(C.c_int)]),
    "ctk_profile_read": (C.c_int, [_P(ProfileRow), C.c_int, _P(C.c_int)]),
    "ctk_probe_mfma": (C.c_int, [C.c_int, C.c_int, _fp, _P(C.c_double), _fp]),
}

_lib = None


def load():
    """Load libctk_hip.so (once) and type every exported symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built.  Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C co-tracker_amd/csrc`).  There is no CPU fallback.")
    # torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  It must be mapped BEFORE our
    # library so that both share ONE HIP runtime; loaded the other way round the process ends up
    # with two runtimes and ours sees no device (hipErrorNoDevice).
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.ctk_abi_version() != ABI_VERSION:
        raise RuntimeError("libctk_hip.so ABI version mismatch")
    _lib = lib
    return lib


class option:
    """`with option(OPT_CORR_VERSION, 1): ...` -- set a back-end option (include/ctk.h: ctk_set_option) for a scope and restore the
    previous value afterwards.  Process-wide (the table is one per loaded library): meant for tests and A/B tools."""

    def __init__(self, key: int, value: int):
        self.key, self.value, self.old = key, value, None

    def __enter__(self):
        lib = load()
        old = C.c_int(0)
        check(lib.ctk_get_option(self.key, C.byref(old)), "ctk_get_option")
        self.old = old.value
        check(lib.ctk_set_option(self.key, self.value), f"ctk_set_option({self.key}, {self.value})")
        return self

    def __exit__(self, *exc):
        load().ctk_set_option(self.key, self.old)
        return False


def option_values() -> tuple:
    """The whole option table (ctk_get_option of every key).  A captured window graph bakes in the values read while it
    was captured (include/ctk.h), so the host models make this tuple part of their graph cache key: changing an option
    re-captures instead of replaying a graph that still runs the old choice."""
    lib = load()
    v = C.c_int(0)
    out = []
    for k in range(OPT_COUNT):
        check(lib.ctk_get_option(k, C.byref(v)), "ctk_get_option")
        out.append(v.value)
    return tuple(out)


def check(rc: int, what: str):
    if rc != 0:
        msg = load().ctk_error_string(rc)
        raise RuntimeError(f"{what} failed: {msg.decode() if msg else rc} (code {rc})")
