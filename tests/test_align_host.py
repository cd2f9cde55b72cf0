"""The arithmetic of the align kernel (csrc/align.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/align_math.h holds the rules of ctk_fit_align -- the correspondence test, the three-point candidate, the pixel and
depth test without a division, the three fixed-point Gauss-Newton rounds on seven parameters through ctk_plane_solve -- in host/device
inline functions.  This test compiles that header with g++ (-ffp-contract=off, the flag the device translation unit is built with)
behind plain loops (tests/host/align_host.cpp) and compares it with the numpy restatement of tests/align_reference.py: every bit of all
five outputs, on the shapes the kernel is held to by tests/test_gpu_align.py and on randomised inputs.  The same file, built as a
stand-alone program under AddressSanitizer and UBSan, runs clean.  The last tests measure what the rules are worth on planted scenes
through the g++ build, against a float64 reference."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import align_reference as AL
from ctk_support import ROOT, host_library

NAMES = ("sim", "scale", "label", "error", "stats")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "align")
    lib.host_align_candidate.restype = C.c_int
    lib.host_align_candidate.argtypes = [C.c_void_p] * 3
    lib.host_fit_align.restype = C.c_int
    lib.host_fit_align.argtypes = [C.c_int] * 4 + [C.c_uint32] + [C.c_float] * 6 + [C.c_void_p] * 10
    return lib


def run_host(host, a, valid_a, b, valid_b, cam, mask=None, tol=2.0, depth_tol=0.1, hypotheses=256, min_points=8, seed=0):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    G, N, _ = a.shape
    keep = [a, np.ascontiguousarray(valid_a, dtype=np.int8), b, np.ascontiguousarray(valid_b, dtype=np.int8)]
    keep.append(None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8))
    before = [None if k is None else k.copy() for k in keep]
    sim = np.full((G, 3, 4), np.nan, dtype=np.float32)
    scale = np.full(G, np.nan, dtype=np.float32)
    label = np.full((G, N), 77, dtype=np.int8)
    error = np.full((G, N), 77.0, dtype=np.float32)
    stats = np.full((G, 4), -99, dtype=np.int32)
    rc = host.host_fit_align(G, N, min_points, hypotheses, seed, *cam, tol, depth_tol, *(None if k is None else k.ctypes.data for k in keep),
                             sim.ctypes.data, scale.ctypes.data, label.ctypes.data, error.ctypes.data, stats.ctypes.data)
    assert rc == 0
    for k, bf in zip(keep, before):  # the inputs are only read
        assert bf is None or np.array_equal(k.view(np.uint8), bf.view(np.uint8))
    return sim, scale, label, error, stats


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def stated_forms(sim, scale, label, error, stats, K):
    """Nothing but the stated forms: labels -1 / 0 / 1; an error of -1 exactly where the label is -1 or the pair has no fit, never a
    NaN; a no-fit pair is all zero with stats (M, 0, -1, bits); a fitted pair has a finite transform, s > 0 and a winner in 0 .. K."""
    assert np.isin(label, (-1, 0, 1)).all() and not np.isnan(error).any()
    for g in range(sim.shape[0]):
        M, ones, k, bits = stats[g].tolist()
        assert 0 <= M <= AL.LIST_MAX and bits & ~(2 | 4 | 8 | 32) == 0 and ones == int((label[g] == 1).sum())
        if k < 0:
            assert (sim[g] == 0).all() and scale[g] == 0 and ones == 0 and (error[g] == -1).all() and bits & 6 == 0
        else:
            assert np.isfinite(sim[g]).all() and scale[g] > 0 and k <= K and M >= 3
            assert ((error[g] == -1) == (label[g] == -1)).all() and (error[g][label[g] >= 0] >= 0).all()
            if bits & 32:
                assert np.array_equal(sim[g], np.eye(3, 4, dtype=np.float32)) and scale[g] == 1 and k == K


def test_candidates_on_edge_values(host):
    """One candidate at a time: planted triples over the whole range of scales and turns, and the triples that must be skipped."""
    rng = np.random.default_rng(0)
    triples = []
    for i in range(60):
        X = np.stack([rng.uniform(-4, 4, 3), rng.uniform(-2, 2, 3), rng.uniform(3, 12, 3)], axis=1).astype(np.float32).astype(np.float64)
        s = float(np.exp(rng.uniform(np.log(0.01), np.log(100.0))))
        Rm, t = AL.rotation(rng.normal(size=3), rng.uniform(0, 3.1)), rng.uniform(-3, 3, 3)
        triples.append((X, (s * X @ Rm.T + t).astype(np.float32).astype(np.float64)))
    X, Y = triples[0]
    line = X[0] + np.arange(3)[:, None] * np.array([0.25, 0.5, 0.125])
    triples += [(line, Y), (X, line), (np.stack([X[0], X[0], X[2]]), Y), (X, np.stack([Y[0], Y[1], Y[1]])), (X * 0.0, Y), (X, Y * 0.0),
                (X * 1e-30, Y), (X * 1e30, Y), (X * 1e-200, Y * 1e200), (X * 1e200, Y), (X, Y[::-1].copy()), (X, -Y), (X, X), (X * 2 ** 20, Y)]
    made = 0
    for X, Y in triples:
        Xa, Ya = np.ascontiguousarray(X, dtype=np.float64).reshape(9), np.ascontiguousarray(Y, dtype=np.float64).reshape(9)
        out = np.full(13, 7.0)
        ok = host.host_align_candidate(Xa.ctypes.data, Ya.ctypes.data, out.ctypes.data)
        want = AL.candidate([[float(v) for v in row] for row in X], [[float(v) for v in row] for row in Y])
        assert bool(ok) == (want is not None)
        sw, Rw, tw = want if want is not None else AL.EYE
        assert np.array_equal(out.view(np.int64), np.array([sw] + list(Rw) + list(tw)).view(np.int64))
        made += ok
    assert 60 <= made <= len(triples) - 6  # the planted ones stand, the degenerate ones are skipped


CASES = {name: (args, kw) for name, args, kw in AL.cases()}
WANT = {}


def want_of(name):
    """The restatement's outputs (and details), computed once and shared."""
    if name not in WANT:
        args, kw = CASES[name]
        details = {}
        WANT[name] = (AL.fit_align(*args, details=details, **kw), details)
    return WANT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_bit_for_bit(host, name):
    args, kw = CASES[name]
    want = want_of(name)[0]
    same(run_host(host, *args, **kw), want)
    stated_forms(*want, kw["hypotheses"])


@pytest.mark.parametrize("seed", range(12))
def test_randomised_bit_for_bit(host, seed):
    """Randomised sizes, batches, cameras, tolerances, masks, spoiled points and validity bytes."""
    rng = np.random.default_rng(100 + seed)
    G, N = int(rng.integers(1, 4)), int(rng.integers(3, 400))
    prs = [AL.pair(1000 * seed + g, N, share=float(rng.uniform(0, 0.7)), plane=bool(rng.integers(0, 2))) for g in range(G)]
    a, b = AL.stack(prs)
    a, b = a.copy(), b.copy()
    for arr in (a, b):
        hit = rng.uniform(size=arr.shape) < 0.01
        arr[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e6, -1.0, 0.0], dtype=np.float32), size=int(hit.sum()))
    va, vb = (rng.uniform(size=(G, N)) < 0.95).astype(np.int8) * 3, (rng.uniform(size=(G, N)) < 0.95).astype(np.int8)
    mask = (rng.uniform(size=(G, N)) < 0.8).astype(np.uint8) if seed % 2 else None
    cam = (float(rng.uniform(500, 1500)), float(rng.uniform(500, 1500)), float(rng.uniform(800, 1100)), float(rng.uniform(400, 700)))
    kw = dict(mask=mask, tol=float(rng.uniform(0.5, 4.0)), depth_tol=float(rng.uniform(0.02, 0.3)), hypotheses=int(rng.integers(1, 200)),
              min_points=int(rng.integers(3, 12)), seed=int(rng.integers(0, 2 ** 31)))
    want = AL.fit_align(a, va, b, vb, cam, **kw)
    same(run_host(host, a, va, b, vb, cam, **kw), want)
    stated_forms(*want, kw["hypotheses"])


def test_cases_cover_what_they_name():
    """The cases reach the branches they are there for (on the restatement, which the two builds equal)."""
    st = {name: want_of(name)[0][4] for name in CASES}
    assert st["size_3"][0].tolist()[:2] == [3, 3] and st["size_3"][0, 2] >= 0
    assert st["size_7"][0].tolist() == [7, 0, -1, 0] and st["size_8"][0, 2] >= 0 and st["size_8"][0, 1] == 8
    for N in (63, 64, 65, 256, 257, 600, 4096, 8192):  # (255 has ONE hypothesis: whatever it gives)
        assert st["size_%d" % N][0, 2] >= 0 and st["size_%d" % N][0, 3] & 2 == 0, N
    assert st["size_4096"][0, 0] == 4096 and st["size_4096"][0, 3] & 8 == 0
    assert st["size_4097"][0, 0] == 4096 and st["size_4097"][0, 3] & 8 and st["size_8192"][0, 3] & 8
    assert st["size_8192"][0, 1] > 4096  # beyond the cap: classified too
    (sim, sc, la, er, s3), _ = want_of("batch_spoiled")
    assert s3[0, 2] >= 0 and s3[1, 2] == -1 and s3[2, 2] >= 0 and (sim[1] == 0).all() and sc[1] == 0  # a no-fit pair between fitted ones
    assert (la[0, [5, 6, 7, 8, 9, 10, 11, 12, 13]] == -1).all() and (la[0, 30:34] == -1).all() and (la[2, 40:45] == -1).all() and la[2, 20] >= 0
    assert (la[1] == 0).all() and (er[1] == -1).all()
    (_, _, la_m, _, s3m), _ = want_of("batch_spoiled_mask")
    assert s3m[0, 0] < s3[0, 0] and s3m[0, 2] >= 0 and ((la_m == -1) == (la == -1)).all()  # the mask thins the list, not the classification
    for name in ("valid_a_zero", "valid_b_zero"):
        out = want_of(name)[0]
        assert (out[4] == [0, 0, -1, 0]).all() and (out[2] == -1).all() and (out[3] == -1).all()
    (_, _, _, _, s3), det = want_of("degenerate_triples")
    assert 0 < det[0]["made"] < 128 and 0 <= s3[0, 2] < 128  # some triples are skipped, a clean one wins
    (_, _, _, _, s3), det = want_of("all_skipped_2")
    assert det[0]["made"] == 0 and s3[0].tolist() == [40, 0, -1, 0]  # nothing but (1, I, 0) is scored, and it has no fit
    (_, _, _, _, s3), det = want_of("all_skipped_1000000")
    assert det[0]["made"] == 0 and s3[0, 2] == 70 and s3[0, 0] == 40  # ... and with wide tolerances it wins
    (_, _, _, _, s3), det = want_of("ties")
    counts = det[0]["counts"]
    assert counts.count(max(counts)) > 1 and s3[0, 2] == counts.index(max(counts)) and s3[0, 1] == 6  # ties go to the lowest k
    assert st["coplanar"][:, 2].min() >= 0 and (st["coplanar"][:, 3] == 0).all()
    assert st["left_out"][0, 3] & 4 and st["left_out"][0, 2] >= 0


def test_identical_sets_give_the_exact_identity(host):
    """Identical structures: exactly s = 1, R = I, t = 0 after the three rounds (all residuals are 0, so the solve returns zero
    increments), every correspondence labelled 1 with error 0."""
    args, kw = CASES["identical"]
    for out in (want_of("identical")[0], run_host(host, *args, **kw)):
        sim, sc, la, er, st = out
        assert np.array_equal(sim[0].view(np.int32), np.eye(3, 4, dtype=np.float32).view(np.int32)) and sc.view(np.int32)[0] == 0x3F800000
        assert st[0].tolist() == [200, 200, kw["hypotheses"], 32] and (la == 1).all() and (er == 0).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/host/align_host.cpp as a program with its own main, built with -fsanitize=address,undefined: it runs the same function over
    spoiled inputs with 3 to 4200 points (the list cap among them), with and without a mask, and must exit clean."""
    exe = str(tmp_path / "align_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DALIGN_HOST_MAIN", "-o", exe, os.path.join(ROOT, "tests", "host", "align_host.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert run.returncode == 0, run.stderr[-2000:]
    assert "rows fitted" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- what the rules are worth: planted scenes through the g++ build -----------------------------------------------------------------------
KINDS = {"400_30": dict(N=400, share=0.3), "400_60": dict(N=400, share=0.6), "40_30": dict(N=40, share=0.3), "40_60": dict(N=40, share=0.6),
         "plane": dict(N=400, share=0.3, plane=True)}
SEEDS = 20
# the default of ops.fit_align and align() on every kind but one: with 16 unmoved points of 40, 256 triples leave 5 of the 20 scenes
# without a fit (three clean points in 6 % of the triples, and a three-point candidate feels its points' depth noise), so that kind is
# held at the most a call takes
HYPOTHESES = {"400_30": 256, "400_60": 256, "40_30": 256, "40_60": 1024, "plane": 256}


def scene_results(host, kind):
    """Every seed of a kind -> rows of (the rules' distance from the truth, the reference's, the rules' distance from the reference,
    unmoved points the reference keeps, those of them the rules drop, moved points kept beyond 4 tol by the rules, by the reference,
    unmoved points within tolerance under the planted transform, those of them the reference drops)."""
    rows = []
    for seed in range(SEEDS):
        sc = AL.planted(seed, **KINDS[kind])
        N = sc["a"].shape[0]
        ones = np.ones((1, N), dtype=np.int8)
        sim, scale, la, er, st = run_host(host, sc["a"][None], ones, sc["b"][None], ones, AL.CAM, hypotheses=HYPOTHESES[kind], min_points=8, seed=0)
        assert st[0, 2] >= 0 and st[0, 3] == 0, (kind, seed, st[0])  # a fit, and no round falls back
        truth = (sc["s"], sc["R"], sc["t"])
        ref, inl = AL.reference(sc["a"], sc["b"], AL.CAM, truth)
        mine = AL.from_sim(sim[0], scale[0])
        ref_inl = AL.reference(sc["a"], sc["b"], AL.CAM, ref, iters=0)[1]  # the points the converged reference keeps
        kept = la[0] == 1
        far = lambda keep, c: int((keep & sc["moved"] & (pixel_distance(c, sc) > 8.0)).sum())
        rows.append((AL.distance(mine, truth), AL.distance(ref, truth), AL.distance(mine, ref), int((ref_inl & ~sc["moved"]).sum()),
                     int((ref_inl & ~sc["moved"] & ~kept).sum()), far(kept, mine), far(ref_inl, ref), int((inl & ~sc["moved"]).sum()),
                     int((inl & ~sc["moved"] & ~ref_inl).sum())))
    return rows


def pixel_distance(c, sc):
    X, Y = sc["a"].astype(np.float64), sc["b"].astype(np.float64)
    Z = c[0] * X @ np.asarray(c[1]).T + c[2]
    px = lambda P: np.stack([AL.CAM[0] * P[:, 0] / P[:, 2], AL.CAM[1] * P[:, 1] / P[:, 2]], axis=1)
    return np.sqrt(((px(Z) - px(Y)) ** 2).sum(axis=1))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_planted_scenes(host, kind):
    """The 1080p scenes of tests/test_resection_host.py with a second structure (align_reference.planted): focal length 1000 px, 400 or
    40 points 3..12 deep (plane: 400 on a slanted plane), a random similarity of scale 0.2..5, up to 30 degrees and up to 3 units,
    0.5 % depth noise and 0.1 px ray noise in both sets, 30 % or 60 % of the common points moved by 12..80 px between the two; 20
    seeds a kind, through the g++ build (tol 2, depth_tol 0.1, min_points 8; the default 256 hypotheses, 1024 for the kind of 40 points
    with 60 % moved: HYPOTHESES has the reason).

    The reference: float64 Umeyama (SVD) over the inliers of the planted transform, refined by converged Gauss-Newton on the rules'
    residual (pixel differences over tol, relative depth difference over depth_tol) over the same inliers.  Conditions: every scene has
    a fit and no round falls back; of the unmoved points the reference keeps at most 1 % are dropped; no moved point further than 4 tol
    (8 px) under the fitted transform is kept -- the reference itself is held to both first: it drops at most 1 % of the unmoved points
    that lie within tolerance under the planted transform, and keeps no moved point beyond 4 tol.  Accuracy: per scene, scale, rotation and translation lie no further from the planted truth than the
    reference does plus the reference's own seed-to-seed spread (the standard deviation of its distance over the 20 seeds of the
    kind): three rounds against convergence and float32 outputs are what separate the two.  The measured values are in
    profiles/align_scenes.json (test_profile_is_current holds them to this function)."""
    rows = scene_results(host, kind)
    ref = np.array([r[1] for r in rows])
    spread = ref.std(axis=0)
    kept = sum(r[3] for r in rows)
    assert sum(r[6] for r in rows) == 0, "the reference keeps a moved point beyond 4 tol: change the kind"
    assert sum(r[8] for r in rows) <= 0.01 * sum(r[7] for r in rows), "the reference drops unmoved points of the planted transform: change the kind"
    assert sum(r[5] for r in rows) == 0 and sum(r[4] for r in rows) <= 0.01 * kept, (kind, [r[4:] for r in rows])
    for seed, r in enumerate(rows):
        for i, what in enumerate(("scale", "rotation", "translation")):
            assert r[0][i] <= r[1][i] + spread[i], (kind, seed, what, r[0][i], r[1][i], spread[i])


def measured(host):
    out = {}
    for kind in sorted(KINDS):
        rows = scene_results(host, kind)
        mine, ref, diff = (np.array([r[i] for r in rows]) for i in range(3))
        out[kind] = dict(scenes=len(rows), hypotheses=HYPOTHESES[kind], **KINDS[kind],
                         worst_rules=dict(zip(("scale_rel", "rotation_deg", "translation"), (float("%.3g" % v) for v in mine.max(axis=0)))),
                         worst_reference=dict(zip(("scale_rel", "rotation_deg", "translation"), (float("%.3g" % v) for v in ref.max(axis=0)))),
                         reference_spread=dict(zip(("scale_rel", "rotation_deg", "translation"), (float("%.3g" % v) for v in ref.std(axis=0)))),
                         largest_difference=dict(zip(("scale_rel", "rotation_deg", "translation"), (float("%.3g" % v) for v in diff.max(axis=0)))),
                         unmoved_kept_by_reference=sum(r[3] for r in rows), of_them_dropped=sum(r[4] for r in rows),
                         unmoved_within_tolerance_of_the_truth=sum(r[7] for r in rows), of_them_dropped_by_reference=sum(r[8] for r in rows))
    out["40_30"]["textbook_residual"] = textbook_figures()
    return out


def textbook_figures():
    """The 40-point, 30 % kind under a float64 reference whose residual is (Z - Y) / Y_z, three numbers weighted alike (Umeyama, then
    converged Gauss-Newton over the inliers of the planted transform) -> how many unmoved points lie within tolerance under the truth,
    how many of them that fit drops, its worst rotation error and pixel distance of an unmoved point."""
    within = dropped = 0
    rot = px = 0.0
    for seed in range(SEEDS):
        sc = AL.planted(seed, **KINDS["40_30"])
        truth = (sc["s"], sc["R"], sc["t"])
        ref, inl = AL.reference(sc["a"], sc["b"], AL.CAM, truth, textbook=True)
        keeps = AL.reference(sc["a"], sc["b"], AL.CAM, ref, iters=0)[1]
        unmoved = inl & ~sc["moved"]
        within, dropped = within + int(unmoved.sum()), dropped + int((unmoved & ~keeps).sum())
        rot, px = max(rot, AL.distance(ref, truth)[1]), max(px, float(pixel_distance(ref, sc)[unmoved].max()))
    return dict(unmoved_within_tolerance_of_the_truth=within, of_them_dropped=dropped, worst_rotation_deg=float("%.3g" % rot),
                worst_pixel_distance_of_an_unmoved_point=float("%.3g" % px))


def test_the_textbook_residual():
    """Why the refit does not minimise (Z - Y) / Y_z as three numbers alike: noise along a point's ray has sideways components in 3-D,
    so on the 40-point kind the CONVERGED float64 fit of that residual over the planted inliers itself drops far more than 1 % of the
    unmoved points at tol = 2 -- the condition every kind is held to -- where the reference on the rules' residual drops none
    (test_planted_scenes).  The figures are in profiles/align_scenes.json."""
    t = textbook_figures()
    print(t)
    assert t["of_them_dropped"] > 0.05 * t["unmoved_within_tolerance_of_the_truth"] and t["worst_pixel_distance_of_an_unmoved_point"] > 2.0


def test_profile_is_current(host):
    """profiles/align_scenes.json holds what test_planted_scenes measures (written by `python tests/test_align_host.py`)."""
    with open(os.path.join(ROOT, "profiles", "align_scenes.json")) as f:
        kept, now = json.load(f)["kinds"], measured(host)
    assert sorted(kept) == sorted(now)
    for kind in now:
        for key, val in now[kind].items():
            if key == "largest_difference":  # rounding of the float32 outputs: its size, not its digits
                assert all(v < 1e-5 and kept[kind][key][k] < 1e-5 for k, v in val.items()), (kind, val)
            elif key == "textbook_residual":
                assert all(abs(v - kept[kind][key][k]) <= 0.05 * abs(v) for k, v in val.items()), (kind, key, val, kept[kind][key])
            elif isinstance(val, dict):  # three digits are kept; a float64 library may move the last one
                assert all(abs(v - kept[kind][key][k]) <= 0.02 * abs(v) for k, v in val.items()), (kind, key, val, kept[kind][key])
            else:
                assert val == kept[kind][key], (kind, key)


if __name__ == "__main__":
    import tempfile

    class _Factory:
        def mktemp(self, name):
            return tempfile.mkdtemp(prefix=name)
    lib = host_library(_Factory(), "align")
    lib.host_fit_align.restype = C.c_int
    lib.host_fit_align.argtypes = [C.c_int] * 4 + [C.c_uint32] + [C.c_float] * 6 + [C.c_void_p] * 10
    doc = dict(what="ctk_fit_align's rules (csrc/align_math.h, g++ build) on align_reference.planted scenes against the float64 reference "
                    "(Umeyama, then converged Gauss-Newton over the same inliers); distances from the planted truth; tol 2, depth_tol 0.1, min_points 8, "
                    "hypotheses per kind; textbook_residual: the same reference on (Z - Y) / Y_z as three numbers alike", kinds=measured(lib))
    with open(os.path.join(ROOT, "profiles", "align_scenes.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
