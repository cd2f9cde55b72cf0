"""The arithmetic of the resection kernel (csrc/resection.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/resection_math.h holds the rules of ctk_fit_resection -- the seed, the one-scalar candidates, the reprojection test,
the three fixed-point Gauss-Newton rounds through ctk_plane_solve -- in host/device inline functions.  This test compiles that header
with g++ (-ffp-contract=off, the flag the device translation unit is built with) behind plain loops (tests/host/resection_host.cpp) and
compares it with the numpy restatement of tests/resection_reference.py: every bit of all four outputs, on the shapes the kernel is held
to by tests/test_gpu_resection.py.  The same file, built as a stand-alone program under AddressSanitizer and UBSan, runs clean.  The
last test measures what the rules are worth on planted camera paths through the g++ builds of all three headers, chained as
CoTrackerOnlinePredictor.localize chains the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_reference as R
import pose_reference as PZ
import resection_reference as RR
from ctk_support import ROOT, host_library

NAMES = ("pose", "label", "error", "stats")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "resection")
    lib.host_resection_seed.restype = None
    lib.host_resection_seed.argtypes = [C.c_void_p] * 2
    lib.host_fit_resection.restype = C.c_int
    lib.host_fit_resection.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 8 + [C.c_void_p] * 14
    return lib


@pytest.fixture(scope="module")
def pose_host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "pose")
    lib.host_fit_pose.restype = C.c_int
    lib.host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    return lib


@pytest.fixture(scope="module")
def epi_host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "epipolar")
    lib.host_fit_epipolar.restype = C.c_int
    lib.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    return lib


def run_host(host, coords, cam, structure, valid, seeds, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0,
             F=1, to=None, lag=None, anchor=None, tol=2.0, hypotheses=256, seed=0, min_points=16, scale=(1.0, 1.0)):
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    G, R_, N, _ = coords.shape
    N_out = N if N_out is None else N_out

    def ptr(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=dt)
        return a, a.ctypes.data
    keep = [ptr(visible, np.uint8), ptr(vis, np.float32), ptr(conf, np.float32), ptr(first_row, np.int32),
            ptr(None if anchor is None else anchor[0], np.float32), ptr(None if anchor is None else anchor[1], np.uint8),
            ptr(structure, np.float32), ptr(valid, np.int8), ptr(seeds, np.float32)]
    before = [None if k[0] is None else k[0].copy() for k in keep]
    pose = np.full((G, F, 3, 4), np.nan, dtype=np.float32)
    label = np.full((G, F, N_out), 77, dtype=np.int8)
    error = np.full((G, F, N_out), 77.0, dtype=np.float32)
    stats = np.full((G, F, 4), -99, dtype=np.int32)
    rc = host.host_fit_resection(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag,
                                 0 if anchor is None else anchor[2], min_points, hypotheses, seed, *cam, scale[0], scale[1], thresh, tol,
                                 coords.ctypes.data, *(k[1] for k in keep), pose.ctypes.data, label.ctypes.data, error.ctypes.data,
                                 stats.ctypes.data)
    assert rc == 0
    for k, b in zip(keep, before):  # the inputs are only read
        assert b is None or np.array_equal(k[0].view(np.uint8), b.view(np.uint8))
    return pose, label, error, stats


def same(got, want):
    for g_, w_, name in zip(got, want, NAMES):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape, name
        eq = (g_.view(np.int32) if g_.dtype == np.float32 else g_) == (w_.view(np.int32) if w_.dtype == np.float32 else w_)
        assert eq.all(), (name, np.argwhere(~eq)[:5].tolist(), g_[~eq][:5], w_[~eq][:5])


def stated_forms(pose, label, error, stats, K):
    """Nothing but the stated forms: labels -1 / 0 / 1; an error of -1 exactly where the label is -1 or the row has no fit, never a
    NaN; a no-fit row is (I | 0) with stats (M, 0, -1, bits); a fitted row has a finite pose and a winner in 0 .. K + 2."""
    assert np.isin(label, (-1, 0, 1)).all() and not np.isnan(error).any()
    eye = np.eye(3, 4, dtype=np.float32)
    for g in range(pose.shape[0]):
        for f in range(pose.shape[1]):
            M, ones, k, bits = stats[g, f].tolist()
            assert 0 <= M <= RR.LIST_MAX and bits & ~63 == 0 and ones == int((label[g, f] == 1).sum())
            if k < 0:
                assert np.array_equal(pose[g, f], eye) and ones == 0 and (error[g, f] == -1).all() and bits & 23 == 0
            else:
                assert np.isfinite(pose[g, f]).all() and k <= K + 2 and ones >= 0
                assert ((error[g, f] == -1) == (label[g, f] == -1)).all() and (error[g, f][label[g, f] >= 0] >= 0).all()
                if bits & 32:
                    assert np.array_equal(pose[g, f], eye) and k == K + 2 and bits & 23 == 0


def test_seeds_on_edge_values(host):
    rng = np.random.default_rng(0)
    from epipolar_reference import rotation
    seeds = [np.eye(3, 4), np.zeros((3, 4)), np.full((3, 4), np.nan), np.full((3, 4), 3e38), np.full((3, 4), 1e-30),
             np.concatenate([np.diag([1.0, -1.0, 1.0]), np.ones((3, 1))], axis=1), np.concatenate([np.eye(3), [[np.inf], [0], [0]]], axis=1),
             np.concatenate([rotation(0.3, -0.2, 1.0) * 1.2, [[0.0], [0.0], [0.0]]], axis=1), np.ones((3, 4))]
    seeds += [np.concatenate([rotation(*rng.uniform(-3, 3, 3)) + rng.normal(0, 0.05, (3, 3)), rng.normal(0, 1, (3, 1))], axis=1)
              for _ in range(20)]
    eyes = 0
    for m in seeds:
        m32 = np.ascontiguousarray(m, dtype=np.float32)
        out = np.full(12, 7.0)
        host.host_resection_seed(m32.ctypes.data, out.ctypes.data)
        Rw, tw = RR.seed_pose(m32)
        assert np.array_equal(out.view(np.int64), np.array(list(Rw) + list(tw)).view(np.int64))
        eyes += (Rw, tw) == RR.EYE
    assert 5 <= eyes < len(seeds)


CASES = {name: (args, kw) for name, args, kw in RR.cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_bit_for_bit(host, name):
    args, kw = CASES[name]
    want = RR.fit_resection(*args, **kw)
    same(run_host(host, *args, **kw), want)
    stated_forms(*want, kw["hypotheses"])


def test_cases_cover_what_they_name():
    """The cases reach the branches they are there for (on the restatement, which the two builds equal)."""
    out = {name: RR.fit_resection(*args, **kw) for name, (args, kw) in CASES.items() if not name.startswith("size_")}
    po, la, er, st = out["anchor_ring"]
    assert (st[0, :, 2] >= 0).sum() >= 2 and (la[1, :, 7] == -1).all() and (la[0, :, 4] == -1).all()  # released slot, empty slot
    assert (la[0, :, [5, 6, 8, 12 + 2, 12 + 5]] == -1).all() and (la[0, :, [12, 13, 15, 16]] >= 0).any()  # spoiled points, validity bytes
    fitted = st[0, :, 2] >= 0  # a structure point behind the camera: +inf on every fitted row that sees it
    assert np.isinf(er[0, fitted, 10][la[0, fitted, 10] >= 0]).all() and np.isinf(er[0, fitted, 10]).any() and (la[0, :, 10] < 1).all()
    po, la, er, st = out["fixed_to"]
    assert st[:, 1, 3].tolist() == [32, 32] and st[:, 1, 2].tolist() == [3, 3] and (po[:, 1] == np.eye(3, 4)).all()  # the frame itself
    assert (st[:, [0, 2], 2] >= 0).all() and (st[:, [0, 2], 3] == 0).all()
    assert (out["valid_all_zero"][3] == [0, 0, -1, 0]).all() and (out["valid_all_zero"][1] == -1).all()
    assert out["six_points_6"][3][0, 0].tolist()[:2] == [6, 6] and out["six_points_6"][3][0, 0, 2] >= 0
    assert out["six_points_5"][3][0, 0].tolist() == [5, 0, -1, 0] and (out["six_points_5"][1][0, 0] == [0, 0, 0, -1, 0, 0]).all()
    st = out["fixed_candidates"][3]
    assert st[1, 0, 2] == 4 and st[1, 1, 2] == 4 and st[1, 2, 2] == 6  # ties go to the lowest of the fixed candidates; with t0 = 0
    # the candidates 4 and 5 are one pose, which (I, 0) beats here: 5 can never win
    assert (out["cap_leaves_out"][3][0, :, 3] == 23).all() and (out["cap_leaves_out"][3][0, :, 2] >= 0).all()
    st = out["lag_wrap_logits"][3]
    assert st[0, 0, 2] >= 0 and st[0, 0, 0] > 200
    args, kw = CASES["size_8192_1_33"]
    st = RR.fit_resection(*args, **kw)[3]
    assert st[0, 0, 0] == 4096 and st[0, 0, 3] & 8 and st[0, 0, 1] > 4096  # beyond the cap: classified too
    # the cap itself: 4096 entries fill the list, the 4097th overflows it and is classified all the same
    full, over = (RR.fit_resection(*CASES[n][0], **CASES[n][1]) for n in ("cap_4096", "cap_4097"))
    assert (full[1][0, 0] >= 0).all() and (over[1][0, 0] >= 0).all()  # every slot is a structure point with a correspondence
    assert full[3][0, 0, 0] == 4096 and full[3][0, 0, 3] == 0 and full[3][0, 0, 2] >= 0
    assert over[3][0, 0, 0] == 4096 and over[3][0, 0, 3] == 8 and over[3][0, 0, 2] == full[3][0, 0, 2]
    assert np.array_equal(over[0].view(np.int32), full[0].view(np.int32)) and np.array_equal(over[1][0, 0, :4096], full[1][0, 0])
    assert over[1][0, 0, 4096] == 1 and 0 <= over[2][0, 0, 4096] <= 4.0 and over[3][0, 0, 1] == full[3][0, 0, 1] + 1


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/host/resection_host.cpp as a program with its own main, built with -fsanitize=address,undefined: it runs the same function
    over spoiled inputs in every source form, with 6 to 4200 points (the list cap among them), and must exit clean."""
    exe = str(tmp_path / "resection_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DRESECTION_HOST_MAIN", "-o", exe, os.path.join(ROOT, "tests", "host", "resection_host.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert run.returncode == 0, run.stderr[-2000:]
    assert "rows fitted" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- what the rules are worth: planted camera paths through the g++ builds ---------------------------------------------------------------
KINDS = ("sideways", "forward", "few")
CAM = (1000.0, 1000.0, 960.0, 540.0)
T = 12


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def rotation_angle(Ra, Rb):
    """Degrees between two rotations, from the chord: exact to rounding for small angles."""
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0))))))


def reprojection(Rm, t, X, q):
    Xc = X @ Rm.T + t
    return (CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2] - q[:, 0]) ** 2 + (CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3] - q[:, 1]) ** 2


def reference_pose(Rm, t, X, q, steps=30):
    """The float64 reference: plain Gauss-Newton on the reprojection error over the given entries, run to convergence (30 steps from
    the planted pose; the step is below 1e-14 long before), an exact rotation update."""
    for _ in range(steps):
        Xc = X @ Rm.T + t
        iz = 1.0 / Xc[:, 2]
        u, v = Xc[:, 0] * iz, Xc[:, 1] * iz
        r = np.concatenate([CAM[0] * u + CAM[2] - q[:, 0], CAM[1] * v + CAM[3] - q[:, 1]])
        gx = np.stack([CAM[0] * iz, 0 * iz, -CAM[0] * iz * u], axis=1)
        gy = np.stack([0 * iz, CAM[1] * iz, -CAM[1] * iz * v], axis=1)
        J = np.concatenate([np.concatenate([np.cross(Xc, gx), gx], axis=1), np.concatenate([np.cross(Xc, gy), gy], axis=1)], axis=0)
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        U, _, Vt = np.linalg.svd((np.eye(3) + skew(d[:3])) @ Rm)
        Rm, t = U @ Vt, t + d[3:]
    return Rm, t


def centre(Rm, t):
    return -Rm.T @ t


def ratio_error(C, Ct, frames):
    """The largest |log| of (distance between two camera positions / the planted one) over all pairs of `frames`."""
    worst = 0.0
    for i in frames:
        for j in frames:
            if i < j:
                worst = max(worst, abs(float(np.log(np.linalg.norm(C[i] - C[j]) / np.linalg.norm(Ct[i] - Ct[j])))))
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_planted_paths(host, pose_host, epi_host, kind):
    """The planted scenes of the epipolar and pose tests (1080p, focal length 1000 px, depths 3..12 m, 0.1 px noise, 25 % movers in
    three groups; sideways, forward, 90 points) extended to a path of 12 frames (resection_reference.planted_path), 20 seeds each; the
    first of the 12 IS the structure's frame, the last returns to its position with the camera turned.  A planted reconstruct --
    the g++ builds of epipolar_math.h and pose_math.h on the pair, then structure_from_pose -- and then, per frame, the chain of the
    three g++ builds as localize() runs it: epipolar against the anchor with structure.valid as the mask (512 hypotheses, tol 1), pose,
    resection with that pose as the seed (256 hypotheses, tol 2, min_points 16).  The float64 reference is reference_pose over the
    entries the rules labelled 1, started at the planted pose.

    Conditions: no static structure point that lies within tol under the planted pose is labelled 0 on more than 1 % of the (frame,
    point) pairs (the float64 reference itself stays inside that cap: checked first); the structure's own frame gives exactly
    (I | 0); every mover that is kept has an error <= tol^2; no round falls back and the cap leaves nothing out.
    Bounds: per scene, the RMS over the 11 other frames of the camera-position error (in baselines) and of the rotation error against
    the planted path are within 1.10 x the float64 reference's (both fit the same inliers; they differ by three rounds against
    convergence and by float32 outputs); the distance ratios between camera positions are within the reference's, with the same 1.10 allowance and for
    the same reason (the two differ in the last digits either way, so a bare <= would test rounding), and those of pose() alone (each
    frame in a unit of its own, |t| = 1) are not.

    Measured, worst of 20 seeds (rules / reference RMS ratio: position, rotation; largest difference to the reference over all
    frames: position in baselines, rotation in degrees; |log| distance-ratio error: localize / reference / pose() alone):
      sideways  1.0000007  1.0000052   1.6e-04  3.8e-04   0.0618 / 0.0618 / 6.28
      forward   1.0000019  1.0000030   1.4e-04  4.0e-04   0.0225 / 0.0225 / 6.39
      few       1.0000092  1.0000021   2.9e-04  6.5e-04   0.0586 / 0.0586 / 6.22
    The errors against the planted path (RMS position up to 0.10 / 0.043 / 0.10 baselines, rotation up to 0.020 / 0.019 / 0.075 degrees)
    are the structure's -- one noisy pair, never refined -- and not the rules': the reference inherits them to the sixth digit."""
    from test_epipolar_host import run_host as run_epipolar
    from test_pose_host import run_host as run_pose
    worst_pos, worst_rot, diff_pos, diff_rot, ratios = 0.0, 0.0, 0.0, 0.0, np.zeros(3)
    for seed in range(20):
        sc = RR.planted_path(seed, kind, T)
        coords, mover = sc["coords"], sc["mover"]
        N = coords.shape[2]
        visible = np.ones((1, T + 2, N), dtype=np.uint8)
        two_view = dict(K=512, tol=1.0, min_points=16, min_base=16.0, seed=0)
        # reconstruct: the pair (row 0, row 1)
        fu, lab, _, est = run_epipolar(epi_host, coords, visible=visible, f0=1, F=1, lag=1, **two_view)
        assert est[0, 0, 2] >= 0
        _, de, _ = run_pose(pose_host, coords, CAM, fu, lab, visible=visible, f0=1, F=1, lag=1, min_points=16)
        pts, valid = RR.structure_from_pose(coords[0, 1], CAM, de[0, 0], lab[0, 0])
        assert valid.sum() >= 0.6 * N
        # localize: rows 2 .. T + 1 against the anchor taken on row 1
        src = dict(visible=visible, f0=2, F=T, anchor=(coords[:, 1].copy(), visible[:, 1].copy(), 1))
        fu, lab, _, _ = run_epipolar(epi_host, coords, mask=valid[None], **two_view, **src)
        seeds, _, _ = run_pose(pose_host, coords, CAM, fu, lab, mask=valid[None], min_points=16, **src)
        po, la, er, st = run_host(host, coords, CAM, pts[None], valid[None], seeds, tol=2.0, hypotheses=256, seed=0, min_points=16, **src)
        assert np.array_equal(po[0, 0], np.eye(3, 4, dtype=np.float32)) and st[0, 0, 3] == 32  # the structure's own frame: exactly (I | 0)
        assert (st[0, :, 2] >= 0).all() and (st[0, 1:, 3] == 0).all(), (seed, st[0])
        kept = la[0] == 1
        assert (er[0][kept] <= 4.0).all() and (er[0][kept & mover[None]] <= 4.0).all()  # every mover that is kept lies within tol
        ok, q16 = R.quant(coords[0], 1.0)
        assert ok.all()
        q, X = q16 / 16.0, pts.astype(np.float64)
        static = (valid == 1) & ~mover
        pairs = dropped = ref_dropped = 0
        C, Cf, Ct, Cp, rot, rot_f = [], [], [], [], [], []
        for j in range(T):
            Rt, tt = sc["truth"][j, :, :3], sc["truth"][j, :, 3]
            Rm, t = po[0, j, :, :3].astype(np.float64), po[0, j, :, 3].astype(np.float64)
            Rf, tf = reference_pose(Rt.copy(), tt.copy(), X[kept[j]], q[2 + j][kept[j]])
            within = reprojection(Rt, tt, X[static], q[2 + j][static]) <= 4.0
            pairs += int(within.sum())
            dropped += int((within & (la[0, j][static] == 0)).sum())
            ref_dropped += int((within & ~(reprojection(Rf, tf, X[static], q[2 + j][static]) <= 4.0)).sum())
            C.append(centre(Rm, t)), Cf.append(centre(Rf, tf)), Ct.append(centre(Rt, tt))
            Cp.append(centre(seeds[0, j, :, :3].astype(np.float64), seeds[0, j, :, 3].astype(np.float64)))
            rot.append(rotation_angle(Rm, Rt)), rot_f.append(rotation_angle(Rf, Rt))
            diff_pos, diff_rot = max(diff_pos, float(np.linalg.norm(C[-1] - Cf[-1]))), max(diff_rot, rotation_angle(Rm, Rf))
        assert ref_dropped <= 0.01 * pairs, (seed, ref_dropped, pairs)  # the reference itself stays inside the cap on these inputs
        assert dropped <= 0.01 * pairs, (seed, dropped, pairs)
        C, Cf, Ct, Cp = (np.array(a) for a in (C, Cf, Ct, Cp))

        def rms(a):
            return float(np.sqrt((np.asarray(a)[1:] ** 2).mean()))
        pos, pos_f = rms(np.linalg.norm(C - Ct, axis=1)), rms(np.linalg.norm(Cf - Ct, axis=1))
        assert pos <= 1.10 * pos_f and rms(rot) <= 1.10 * rms(rot_f), (seed, pos, pos_f, rms(rot), rms(rot_f))
        worst_pos, worst_rot = max(worst_pos, pos / pos_f), max(worst_rot, rms(rot) / rms(rot_f))
        # the feature's point: distances between camera positions compare across frames (the frames 1 .. T - 2 lie apart from one
        # another; the first and the last sit on the anchor)
        frames = range(1, T - 1)
        r_loc, r_ref, r_pose = ratio_error(C, Ct, frames), ratio_error(Cf, Ct, frames), ratio_error(Cp, Ct, frames)
        assert r_loc <= 1.10 * r_ref and r_pose > r_ref, (seed, r_loc, r_ref, r_pose)
        ratios = np.maximum(ratios, [r_loc, r_ref, r_pose])
    print(kind, "rules / reference RMS ratio: position", worst_pos, "rotation", worst_rot, "; largest difference to the reference:",
          diff_pos, "baselines,", diff_rot, "deg; distance ratios |log| localize / reference / pose():", ratios.tolist())
