"""The six fit kernels decide alike which slots of a history are correspondences (csrc/fit_device.h: fit_gather).  One small history --
two chunks of slots, the second partial, a ring that wraps inside the call, first rows behind the source frame and behind the frame,
positions the quantiser refuses, slots unseen on one of the two frames -- goes through ctk_fit_motion, _objects, _planes, _epipolar,
_pose and _resection under each source form, with `visible` and with the logits; the set of slots each kernel reports as no
correspondence equals, exactly, the set the numpy restatement of tests/objects_reference.py gives.  Nothing else excludes a slot:
resection runs with `valid` all ones, pose with a label of all ones and no mask on frames that all have a fit."""
import numpy as np
import pytest

import motion_reference as R
import objects_reference as O
import resection_reference as RR
import test_gpu_epipolar as TE  # the C-ABI calls on fenced outputs: imported, not restated
import test_gpu_motion as TM
import test_gpu_objects as TO
import test_gpu_planes as TP
import test_gpu_pose as TZ
import test_gpu_resection as TR

G, N, N_OUT, F, ROWS, T, F0 = 2, 320, 300, 3, 8, 9, 6  # frames 6, 7, 8 of a ring of 8 rows after 9 frames: rows 6, 7, 0
SCALE = (1.37, 0.81)
FORMS = {"lag": dict(lag=2), "to": dict(to=3), "anchor": None}  # the anchor was taken on frame 0, which the ring has dropped
NAN_BITS = 0x7FC00000


def history(form, logits):
    """-> (ring coords [G,ROWS,N,2], cam, structure, seeds, the source keywords of every raw_fit and restatement)."""
    sc = RR.scene(17, G, T, N, src=0, p_visible=0.85)
    coords, visible = sc["coords"], sc["visible"]
    rng = np.random.default_rng(5)
    first = np.zeros((G, N), dtype=np.int32)
    late = rng.uniform(size=(G, N)) < 0.2
    first[late] = rng.choice((5, 7, 9), size=int(late.sum()))  # behind the source frame; behind frame 6 as well; behind every frame
    for g in range(G):  # positions that are no positions, on the frame or on its source only
        coords[g, 6, 10 + g], coords[g, 4, 20 + g, 1], coords[g, 8, 30 + g, 0] = np.nan, np.inf, 1e9
        coords[g, 3, 40 + g, 0], coords[g, 0, 50 + g], coords[g, 7, 290 + g, 1] = -1e9, np.nan, -np.inf
    src = dict(first_row=first, N_out=N_OUT, f0=F0, F=F, scale=SCALE)
    src.update(FORMS[form] or dict(anchor=(coords[:, 0].copy(), visible[:, 0].copy(), 0)))
    coords, visible = R.fold(coords, ROWS, T), R.fold(visible, ROWS, T)
    if logits:  # away from the threshold: products of 0.98 or below 0.02 against 0.6, so that expf cannot decide
        src.update(vis=np.where(visible != 0, 5.0, -5.0).astype(np.float32) + rng.uniform(-1, 1, visible.shape).astype(np.float32),
                   conf=np.full(visible.shape, 6.0, dtype=np.float32), thresh=0.6)
    else:
        src.update(visible=visible)
    fx, fy, cx, cy = sc["cam"]
    cam = (SCALE[0] * fx, SCALE[1] * fy, SCALE[0] * cx, SCALE[1] * cy)
    seeds = RR.unit_seeds(sc["truth"], range(F0, F0 + F))
    return coords, cam, sc["structure"], seeds, src


def restated(coords, src):
    """bool [G,F,N_OUT]: slot n of frame f is no correspondence, by the restatement."""
    none = O.fit_objects(coords, L=1, K=1, min_points=1, **src)[1] == -1
    share = 1.0 - none.mean(axis=-1)
    assert (share >= 0.25).all() and (share <= 0.75).all(), share  # agreement is not vacuous on any (group, frame)
    return none


@pytest.mark.gpu
@pytest.mark.parametrize("logits", (False, True), ids=("visible", "logits"))
@pytest.mark.parametrize("form", tuple(FORMS))
def test_the_six_kernels_agree_on_what_is_no_correspondence(form, logits):
    coords, cam, structure, seeds, src = history(form, logits)
    want = restated(coords, src)
    got = {}
    if form == "lag":
        motion_src = {k: v for k, v in src.items() if k != "lag"}
        got["motion"] = TM.raw_fit(coords, lag=src["lag"], K=1, **motion_src)[1] == -1
    got["objects"] = TO.raw_fit(coords, L=1, K=1, min_points=1, **src)[1] == -1
    got["planes"] = TP.raw_fit(coords, K=1, **src)[1] == -1
    fundamental, label, _, stats = TE.raw_fit(coords, min_points=8, K=64, seed=3, min_base=3.0, tol=1.0, **src)
    got["epipolar"] = label == -1
    assert (stats[..., 2] >= 0).all()  # a matrix on every frame, so that pose leaves no correspondence without depths
    _, depth, stats = TZ.raw_fit(coords, cam, fundamental, np.ones((G, F, N_OUT), dtype=np.int8), min_points=8, **src)
    assert (stats[..., 2] >= 0).all()
    bits = depth.view(np.uint32)
    got["pose"] = bits[..., 0] == NAN_BITS
    assert (got["pose"] == (bits[..., 1] == NAN_BITS)).all()
    got["resection"] = TR.raw_fit(coords, cam, structure, np.ones((G, N), dtype=np.int8), seeds, hypotheses=8, min_points=6, **src)[1] == -1
    for name, none in got.items():
        assert none.shape == want.shape and (none == want).all(), (name, np.argwhere(none != want)[:5].tolist())
