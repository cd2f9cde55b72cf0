"""The host layer of the eight fit readers (-m gpu): ops.fit_motion, track_field, fit_objects, fit_planes, fit_epipolar, fit_pose,
fit_resection, fit_structure and the StreamGroups methods of the same names hand the library a struct.  A recorder between ops and
the library copies that struct at every launch; its scalar fields, and where each pointer leads -- into which tensor of the case and
at which byte, to nothing, or to a copy the host layer made itself --, are compared with tests/golden/fit_host_args.json, recorded
with CTK_RECORD_FIT_HOST_ARGS=1 on the commit before the host layer was restated.  A table of refusals, one fault per call and
written out here, says what is refused, with which exception and word, under the reader's own name, and before any launch.  Only
public functions and _lib are used: the file passes unedited on either side of a refactor of ops.py."""
import json
import os

import pytest
import torch

from ctk_support import HW, S, STEP, STRIDE, dev
from ctk_support import lib  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_host_args.json")
RECORD = os.environ.get("CTK_RECORD_FIT_HOST_ARGS") == "1"
ENTRIES = {"motion": "ctk_fit_motion", "field": "ctk_track_field", "objects": "ctk_fit_objects", "planes": "ctk_fit_planes",
           "epipolar": "ctk_fit_epipolar", "pose": "ctk_fit_pose", "resection": "ctk_fit_resection", "structure": "ctk_fit_structure"}
TENSOR_FORM = {"motion": "fit_motion", "field": "track_field", "objects": "fit_objects", "planes": "fit_planes",
               "epipolar": "fit_epipolar", "pose": "fit_pose", "resection": "fit_resection", "structure": "fit_structure"}
READERS = tuple(ENTRIES)
SOURCED = ("field", "objects", "planes", "epipolar", "pose", "resection")  # the readers with a lag / to / anchor form
G, N, N_OUT, T, ROWS, DONE, F0, F = 2, 12, 9, 6, 8, 11, 7, 3  # a ring of 8 rows 11 frames in: frames 7, 8, 9 are rows 7, 0, 1
CAM, SIZE, GRID = (50.0, 52.0, 48.0, 32.0), (64, 96), (5, 7)  # GRID: field_grid(SIZE, 16)
f32, i8, u8, i16, i32, i64 = torch.float32, torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64


class Recorder:
    """Stands where L.load() stands: every symbol is the library's own, the eight entry points copy their args struct first."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in ENTRIES.values():
            return fn

        def entry(ref, *rest):
            a = ref._obj
            self.calls.append((name, type(a).from_buffer_copy(a)))
            return fn(ref, *rest)
        return entry


@pytest.fixture
def rec(lib, monkeypatch):  # noqa: F811
    from cotracker_amd import _lib
    r = Recorder(lib)
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


class Case:
    """The tensors of one call, by name: what a pointer of the struct may lead into."""

    def __init__(self):
        self.named = {}
        self.gen = torch.Generator().manual_seed(3)

    def t(self, name, dtype, *shape):
        if name in ("pose", "seed_pose", "origin"):
            x = torch.eye(3, 4).expand(*shape).contiguous()
        elif dtype == f32:
            x = torch.rand(*shape, generator=self.gen) * 40.0 + 4.0
        elif dtype in (i8, u8, torch.bool):
            x = torch.randint(0, 2, shape, generator=self.gen).to(dtype)
        else:
            x = torch.zeros(*shape, dtype=dtype)
        self.named[name] = x = x.to(dev())
        return x

    def anchor(self, g, coords=(f32, N, 2), visible=(u8, N)):
        from cotracker_amd import ops
        return ops.FieldAnchor(self.t("anchor_coords", coords[0], g, *coords[1:]), self.t("anchor_visible", visible[0], g, *visible[1:]), 1)

    def outs(self, reader, g, f, n, drop=0, dtype=None, shape=None):
        """An `out` tuple of `reader`: as it must be, or `drop` tensors short, or its second tensor of another dtype or shape."""
        spec = [[dt, sh] for dt, sh in OUTS[reader](g, f, n)][:len(OUTS[reader](g, f, n)) - drop]
        spec[1] = [dtype or spec[1][0], shape or spec[1][1]]
        return tuple(self.t(f"out{k}", dt, *sh) for k, (dt, sh) in enumerate(spec))


OUTS = {  # a reader that takes `out` -> (G, F, N_out) -> the (dtype, shape) of its outputs
    "motion": lambda g, f, n: [(f32, (g, f, 2, 3)), (i8, (g, f, n)), (i32, (g, f, 4))],
    "field": lambda g, f, n: [(i32, (g, f, *GRID, 2)), (u8, (g, f, *GRID)), (i32, (g, f, 4))],
    "epipolar": lambda g, f, n: [(f32, (g, f, 3, 3)), (i8, (g, f, n)), (f32, (g, f, n)), (i32, (g, f, 4))],
    "pose": lambda g, f, n: [(f32, (g, f, 3, 4)), (f32, (g, f, n, 2)), (i32, (g, f, 4))],
    "resection": lambda g, f, n: [(f32, (g, f, 3, 4)), (i8, (g, f, n)), (f32, (g, f, n)), (i32, (g, f, 4))],
    "structure": lambda g, f, n: [(f32, (g, n, 3)), (i8, (g, n)), (f32, (g, n)), (i32, (g, n, 4)), (f32, (g, 3, 4))],
}
TAKES_OUT = tuple(OUTS)


def own_inputs(c, reader, g, f, n, axis=True):
    """What a reader takes besides its source, valid: g groups (axis=False: no group axis), f frames, n = N_out points."""
    ga = (g,) if axis else ()
    if reader == "field":
        return dict(size=SIZE, lag=1)
    if reader == "epipolar":
        return dict(min_points=8)
    if reader == "pose":
        return dict(intrinsics=CAM, fundamental=c.t("fundamental", f32, g, f, 3, 3), label=c.t("label", i8, g, f, n), min_points=8)
    if reader == "resection":
        return dict(intrinsics=CAM, structure=c.t("structure", f32, *ga, N, 3), valid=c.t("valid", i8, *ga, N),
                    seed_pose=c.t("seed_pose", f32, *ga, f, 3, 4), min_points=6, hypotheses=16)
    if reader == "structure":
        return dict(intrinsics=CAM, pose=c.t("pose", f32, *ga, f, 3, 4))
    return {}


_stream = []


def stream():
    """A hand-built ring stream 11 frames in: finite positions, positive logits."""
    if not _stream:
        from cotracker_amd import ops
        sizes = [(HW[0] // STRIDE >> l, HW[1] // STRIDE >> l) for l in range(4)]
        gs = ops.StreamGroups(torch.zeros(G, N, 3, device=dev()), S, STEP, STRIDE, sizes, ring_rows=ROWS)
        gen = torch.Generator().manual_seed(5)
        gs.hist[0].copy_(torch.rand(G, ROWS, N, 2, generator=gen) * 40.0 + 4.0)
        gs.hist[1].copy_(torch.rand(G, ROWS, N, generator=gen) + 2.0)
        gs.hist[2].copy_(torch.rand(G, ROWS, N, generator=gen) + 2.0)
        gs.committed = DONE
        _stream.append(gs)
    return _stream[0]


class Ctx:
    """What a lazily built argument may look at: the case, the reader and the G, F, N_out of the call."""

    def __init__(self, c, reader, g, f, n):
        self.c, self.reader, self.g, self.f, self.n = c, reader, g, f, n


def call(reader, form, **over):
    """-> (case, thunk): `reader` called validly through `form` ("tensor", "history"), with the arguments of `over` put over the
    valid ones; a callable among them is given the Ctx and returns the argument.  `group`, `squeeze` (tensor form without the group
    axis) and `bool_visible`, `strided` shape the source itself."""
    from cotracker_amd import ops
    c = Case()
    if form == "tensor":
        axis = not over.pop("squeeze", False)
        g, f, n = (G if axis else 1), T, N
        ga = (g,) if axis else ()
        kw = dict(visible=c.t("visible", torch.bool if over.pop("bool_visible", False) else u8, *ga, T, N))
        kw["tracks"] = c.t("tracks", f32, *ga, T, N, 3)[..., :2] if over.pop("strided", False) else c.t("tracks", f32, *ga, T, N, 2)
        kw.update(own_inputs(c, reader, g, f, n, axis))
        fn = getattr(ops, TENSOR_FORM[reader])
    else:
        group = over.get("group")
        g, f, n = (G if group is None else 1), F, N_OUT
        kw = dict(f0=F0, F=F, N_out=N_OUT, **own_inputs(c, reader, g, f, n))
        c.named.update(zip(("hist_coords", "hist_vis", "hist_conf"), stream().hist))
        fn = getattr(stream(), reader)
    ctx = Ctx(c, reader, g, f, n)
    for k, v in over.items():
        kw[k] = v(ctx) if callable(v) else v
    if reader == "field" and ("to" in over or "anchor" in over):
        kw.pop("lag")  # (exactly one of the three)
    return c, lambda: fn(**kw)


# ----------------------------------------------------------------------------------------------------------------------
# the struct of every valid form
# ----------------------------------------------------------------------------------------------------------------------
def labels(name, dtype=i8, flat=False):
    return lambda x: x.c.t(name, dtype, *(() if flat else (x.g,)), N)


def out(x, **wrong):
    return x.c.outs(x.reader, x.g, x.f, x.n, **wrong)


def first_row_i32(x):
    return x.c.t("first_row", i32, G, N)


def first_row_i64(x):
    return x.c.t("first_row", i64, x.g, N)


def anchor(x):
    return x.c.anchor(x.g)


def valid_cases():
    cases = {}
    for r in READERS:
        cases[f"{r}-tensor"] = (r, "tensor", {})
        cases[f"{r}-tensor-squeezed-bool"] = (r, "tensor", dict(squeeze=True, bool_visible=True))
        cases[f"{r}-tensor-strided-first_row"] = (r, "tensor", dict(strided=True, **({} if r == "motion" else dict(first_row=first_row_i64))))
        cases[f"{r}-history"] = (r, "history", {})
        cases[f"{r}-history-group-first_row"] = (r, "history", dict(group=1, first_row=first_row_i32))
        if r in SOURCED:
            cases[f"{r}-tensor-to"] = (r, "tensor", dict(to=2))
            cases[f"{r}-tensor-anchor"] = (r, "tensor", dict(anchor=anchor))
            cases[f"{r}-history-to-group"] = (r, "history", dict(to=4, group=1))
            cases[f"{r}-history-to-first_row"] = (r, "history", dict(to=4, first_row=first_row_i32))
            cases[f"{r}-history-anchor"] = (r, "history", dict(anchor=anchor))
            cases[f"{r}-history-anchor-group"] = (r, "history", dict(anchor=anchor, group=1, first_row=first_row_i32))
        if r in TAKES_OUT:
            cases[f"{r}-tensor-out"] = (r, "tensor", dict(out=out))
            cases[f"{r}-history-out"] = (r, "history", dict(out=out, group=1))
    cases["motion-tensor-frames"] = ("motion", "tensor", dict(first_frame=2, frames=3, lag=2, model="translation", scale=(1.5, 0.5)))
    cases["motion-tensor-frames-short"] = ("motion", "tensor", dict(first_frame=1, frames=2))
    cases["motion-history-options"] = ("motion", "history", dict(lag=2, model="translation", tol=3.0, hypotheses=64, min_base=8.0, seed=7,
                                                                   scale=(1.5, 0.5), thresh=0.4))
    for lag in (-1, -2, 2):
        cases[f"field-tensor-lag{lag}"] = ("field", "tensor", dict(lag=lag, first_frame=1, frames=4, N_out=N_OUT, cell=8, radius=3))
        if lag != -2:  # (frame 9 + 2 has not been tracked)
            cases[f"field-history-lag{lag}"] = ("field", "history", dict(lag=lag, cell=8, radius=3))
    cases["field-tensor-lag-2-tail"] = ("field", "tensor", dict(lag=-2, first_frame=3, frames=3))
    for r, key in (("objects", "objects"), ("planes", "planes")):
        cases[f"{r}-tensor-labels"] = (r, "tensor", {"labels": labels("labels"), key: 2, "frames": (1, 4), "lag": 2})
        cases[f"{r}-tensor-labels-flat"] = (r, "tensor", {"labels": labels("labels", flat=True), key: 2, "to": 5, "frames": (2, 2)})
        cases[f"{r}-history-labels"] = (r, "history", {"labels": labels("labels"), key: 2, "lag": 2, "seed": 9, "min_points": 3})
        cases[f"{r}-history-labels-group"] = (r, "history", {"labels": labels("labels", flat=True), key: 2, "group": 1})
    cases["planes-tensor-inverse"] = ("planes", "tensor", dict(inverse=True, anchor=anchor, tol=1.5, hypotheses=32, min_base=4.0, seed=11))
    cases["objects-tensor-lag-unread"] = ("objects", "tensor", dict(to=1, lag=0, model="translation"))
    for r in ("epipolar", "pose"):
        cases[f"{r}-tensor-mask-flat"] = (r, "tensor", dict(mask=labels("mask", u8, flat=True), lag=2))
        cases[f"{r}-tensor-mask-bool"] = (r, "tensor", dict(mask=labels("mask", torch.bool), to=3))
        cases[f"{r}-history-mask"] = (r, "history", dict(mask=labels("mask", i8), lag=2))
    cases["epipolar-history-options"] = ("epipolar", "history", dict(tol=0.5, hypotheses=64, min_base=4.0, min_points=9, seed=13))
    cases["resection-tensor-seed-wraps"] = ("resection", "tensor", dict(seed=2 ** 32 + 5, tol=1.5, hypotheses=1024))
    cases["resection-history-seed-wraps"] = ("resection", "history", dict(seed=2 ** 32 + 5, lag=2))
    old = dict(pose_stats=lambda x: x.c.t("pose_stats", i32, x.g, x.f, 4), structure=lambda x: x.c.t("structure", f32, x.g, N, 3),
               valid=lambda x: x.c.t("valid", u8, x.g, N), origin=lambda x: x.c.t("origin", f32, x.g, 3, 4), source_frame=2, into=1,
               refine=True, tol=1.5, min_views=2, min_parallax=2.5)
    cases["structure-tensor-old"] = ("structure", "tensor", old)
    cases["structure-history-old"] = ("structure", "history", dict(old, group=1))
    return cases


VALID = valid_cases()


def resolve(p, tensors):
    if not p:
        return None
    for name, x in tensors.items():
        lo = x.untyped_storage().data_ptr()
        if lo <= p < lo + x.untyped_storage().nbytes():
            return [name, p - x.data_ptr()]
    return "copy"


def observe(rec, reader, form, over):
    """One valid call under the recorder -> what the golden file holds of it."""
    import ctypes as C
    c, thunk = call(reader, form, **over)
    got = thunk()
    torch.cuda.synchronize()
    assert isinstance(got, tuple)
    given = [c.named.get(f"out{k}") for k in range(len(got))]
    assert "out" not in over or all(a is b for a, b in zip(got, given))  # the `out` tuple itself comes back
    tensors = dict(c.named, **{f"out{k}": x for k, x in enumerate(got)})
    calls = []
    for name, a in rec.calls:
        scalars, pointers = {}, {}
        for field, kind in a._fields_:
            if kind is C.c_void_p:
                pointers[field] = resolve(getattr(a, field), tensors)
            else:
                scalars[field] = getattr(a, field)
        calls.append({"entry": name, "scalars": scalars, "pointers": pointers})
    return {"calls": calls, "returns": [[str(x.dtype), list(x.shape), x.is_contiguous()] for x in got]}


_golden = {}


def golden():
    if not _golden:
        _golden.update(json.load(open(GOLDEN)))
    return _golden


@pytest.mark.parametrize("case", tuple(VALID))
def test_the_struct_of_a_valid_call_is_the_recorded_one(rec, case):
    got = observe(rec, *VALID[case])
    assert [c["entry"] for c in got["calls"]] == [ENTRIES[VALID[case][0]]]  # one launch of the reader's own entry point
    if RECORD:
        _golden[case] = got
        if len(_golden) == len(VALID):
            with open(GOLDEN, "w") as f:
                json.dump({k: _golden[k] for k in VALID}, f, separators=(",", ":"))
                f.write("\n")
        return
    assert json.loads(json.dumps(got)) == golden()[case]


def test_every_recorded_case_is_still_asked_for():
    assert RECORD or set(golden()) == set(VALID)


@pytest.mark.parametrize("form", ("tensor", "history"))
def test_resection_takes_a_seed_beyond_32_bits_and_keeps_its_low_bits(rec, form):
    _, thunk = call("resection", form, seed=2 ** 32 + 5)
    thunk()
    assert [a.seed for _, a in rec.calls] == [5]


# ----------------------------------------------------------------------------------------------------------------------
# refusals: (readers, forms, the bad argument, exception type, a word of the message) -- one fault per call
# ----------------------------------------------------------------------------------------------------------------------
BOTH, TENSOR, HISTORY = ("tensor", "history"), ("tensor",), ("history",)
SAMPLED = ("motion", "objects", "planes", "epipolar")  # hypotheses up to Motion.HYPOTHESES_MAX = 4096, seed in 0..2^32 - 1
CAMERA = ("pose", "resection", "structure")


def long_views(x):
    return x.c.t("pose", f32, x.g, 257, 3, 4)


REFUSALS = [
    # the source form
    (SOURCED, BOTH, dict(to=2, anchor=anchor), ValueError, "anchor"),
    (SOURCED, BOTH, dict(to=-1), ValueError, "to must be"),
    (SOURCED, TENSOR, dict(to=T), ValueError, "tracked frames"),
    (SOURCED, HISTORY, dict(to=DONE), ValueError, "beyond"),
    (SOURCED, HISTORY, dict(to=2), ValueError, "left the history"),
    (("motion",) + SOURCED, BOTH, dict(lag=0), ValueError, "lag"),
    (SOURCED, BOTH, dict(anchor=lambda x: x.c.anchor(x.g, coords=(f32, N + 1, 2))), ValueError, "anchor"),
    (SOURCED, BOTH, dict(anchor=lambda x: x.c.anchor(x.g, visible=(u8, N, 1))), ValueError, "anchor"),
    (SOURCED, BOTH, dict(anchor=lambda x: x.c.anchor(x.g, coords=(torch.float64, N, 2))), ValueError, "anchor"),
    (SOURCED, BOTH, dict(anchor=lambda x: x.c.anchor(x.g, visible=(i32, N))), ValueError, "anchor"),
    # the per-point lists
    (("objects", "planes"), BOTH, dict(labels=labels("labels", i16)), ValueError, "labels"),
    (("objects", "planes"), BOTH, dict(labels=lambda x: x.c.t("labels", i8, x.g, N + 1)), ValueError, "labels"),
    (("objects", "planes"), BOTH, dict(labels=lambda x: x.c.t("labels", i8, x.g + 1, N)), ValueError, "labels"),
    (("epipolar", "pose"), BOTH, dict(mask=labels("mask", f32)), ValueError, "mask"),
    (("epipolar", "pose"), BOTH, dict(mask=lambda x: x.c.t("mask", u8, x.g, N - 1)), ValueError, "mask"),
    (("epipolar", "pose"), BOTH, dict(mask=lambda x: x.c.t("mask", u8, x.g + 1, N)), ValueError, "mask"),
    # the rounds
    (("objects",), BOTH, dict(objects=0), ValueError, "objects"),
    (("objects",), BOTH, dict(objects=17), ValueError, "objects"),
    (("planes",), BOTH, dict(planes=2), ValueError, "planes"),
    (("objects", "planes"), BOTH, dict(min_points=0), ValueError, "min_points"),
    (("epipolar", "pose"), BOTH, dict(min_points=7), ValueError, "min_points"),
    (("resection",), BOTH, dict(min_points=5), ValueError, "min_points"),
    # the sampling
    (SAMPLED + ("resection",), BOTH, dict(hypotheses=0), ValueError, "hypotheses"),
    (SAMPLED, BOTH, dict(hypotheses=4097), ValueError, "hypotheses"),
    (("resection",), BOTH, dict(hypotheses=1025), ValueError, "hypotheses"),
    (SAMPLED, BOTH, dict(seed=-1), ValueError, "seed"),
    (SAMPLED, BOTH, dict(seed=2 ** 32), ValueError, "seed"),
    (("motion", "objects"), BOTH, dict(model="affine"), ValueError, "model"),
    # the intrinsics
    (CAMERA, BOTH, dict(intrinsics=lambda x: torch.tensor(CAM)), ValueError, "intrinsics"),
    (CAMERA, BOTH, dict(intrinsics=CAM[:3]), ValueError, "intrinsics"),
    (CAMERA, BOTH, dict(intrinsics=(0.0,) + CAM[1:]), ValueError, "intrinsics"),
    (CAMERA, BOTH, dict(intrinsics=CAM[:2] + (float("nan"),) + CAM[3:]), ValueError, "intrinsics"),
    # resection and structure
    (("resection", "structure"), BOTH, dict(tol=0.0), ValueError, "tol"),
    (("resection", "structure"), BOTH, dict(tol=float("inf")), ValueError, "tol"),
    (("structure",), TENSOR, dict(into=T), ValueError, "into"),
    (("structure",), HISTORY, dict(into=F), ValueError, "into"),
    (("structure",), BOTH, dict(structure=lambda x: x.c.t("structure", f32, x.g, N, 3)), ValueError, "valid"),
    (("structure",), BOTH, dict(min_parallax=0.0), ValueError, "min_parallax"),
    (("structure",), BOTH, dict(min_parallax=91.0), ValueError, "min_parallax"),
    (("structure",), BOTH, dict(min_views=1), ValueError, "min_views"),
    (("structure",), TENSOR, dict(tracks=lambda x: x.c.t("tracks", f32, x.g, 257, N, 2), visible=lambda x: x.c.t("visible", u8, x.g, 257, N),
                                   pose=long_views), ValueError, "views"),
    (("structure",), HISTORY, dict(F=257, pose=long_views), ValueError, "views"),
    # whom
    (READERS, HISTORY, dict(N_out=0), ValueError, "N_out"),
    (READERS, HISTORY, dict(N_out=N + 1), ValueError, "N_out"),
    (("field",), TENSOR, dict(N_out=0), ValueError, "N_out"),
    (("field",), TENSOR, dict(N_out=N + 1), ValueError, "N_out"),
    (READERS, HISTORY, dict(group=G), ValueError, "group"),
    (READERS, HISTORY, dict(first_row=lambda x: x.c.t("first_row", i64, G, N)), ValueError, "first_row"),
    # the outputs
    (TAKES_OUT, BOTH, dict(out=lambda x: out(x, drop=1)), ValueError, "out"),
    (TAKES_OUT, BOTH, dict(out=lambda x: out(x, dtype=torch.float64)), ValueError, "out"),
    (TAKES_OUT, BOTH, dict(out=lambda x: out(x, shape=(x.g, x.f + 1, x.n))), ValueError, "out"),
]
REFUSED = [(r, form, k) for k, row in enumerate(REFUSALS) for r in row[0] for form in row[1]]


@pytest.mark.parametrize("reader,form,row", REFUSED, ids=[f"{r}-{form}-{k}-{'-'.join(REFUSALS[k][2])}" for r, form, k in REFUSED])
def test_a_bad_argument_is_refused_under_the_readers_name_before_any_launch(rec, reader, form, row):
    _, _, bad, exc, word = REFUSALS[row]
    _, thunk = call(reader, form, **bad)
    with pytest.raises(exc) as e:
        thunk()
    who = TENSOR_FORM[reader] if form == "tensor" else reader
    assert str(e.value).startswith(who + ":") and word in str(e.value), str(e.value)
    assert rec.calls == []
