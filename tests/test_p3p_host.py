"""The arithmetic of the p3p kernel (csrc/p3p.hip) pinned WITHOUT a GPU.

co-tracker_amd/csrc/p3p_math.h holds what ctk_fit_p3p adds to ctk_fit_resection's rules -- the candidate that three entries of the fit
list fix: the start, six Newton rounds through a cofactor solve, the polar steps -- in host/device inline functions.  This test compiles
that header with g++ (-ffp-contract=off, the flag the device translation unit is built with) behind plain loops
(tests/host/p3p_host.cpp) and compares it with the numpy restatement of tests/p3p_reference.py: every bit of all four outputs, on the
shapes the kernel is held to by tests/test_gpu_p3p.py.  The same file, built as a stand-alone program under AddressSanitizer and UBSan,
runs clean.  The last tests measure what the rules are worth on planted scenes through the g++ build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_reference as R
import p3p_reference as P3
import resection_reference as RR
from ctk_support import ROOT, host_library
from test_resection_host import CAM, KINDS, T, centre, reference_pose, reprojection, rotation_angle, same, stated_forms


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = host_library(tmp_path_factory, "p3p")
    lib.host_p3p_candidate.restype = C.c_int
    lib.host_p3p_candidate.argtypes = [C.c_float] * 4 + [C.c_void_p] * 3
    lib.host_fit_p3p.restype = C.c_int
    lib.host_fit_p3p.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 8 + [C.c_void_p] * 13
    return lib


def run_host(host, coords, cam, structure, valid, visible=None, vis=None, conf=None, thresh=0.0, first_row=None, N_out=None, f0=0, F=1,
             to=None, lag=None, anchor=None, tol=2.0, hypotheses=256, seed=0, min_points=16, scale=(1.0, 1.0)):
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
            ptr(structure, np.float32), ptr(valid, np.int8)]
    before = [None if k[0] is None else k[0].copy() for k in keep]
    pose = np.full((G, F, 3, 4), np.nan, dtype=np.float32)
    label = np.full((G, F, N_out), 77, dtype=np.int8)
    error = np.full((G, F, N_out), 77.0, dtype=np.float32)
    stats = np.full((G, F, 4), -99, dtype=np.int32)
    rc = host.host_fit_p3p(G, N, N_out, R_, f0, F, -1 if to is None else to, 0 if lag is None else lag,
                           0 if anchor is None else anchor[2], min_points, hypotheses, seed, *cam, scale[0], scale[1], thresh, tol,
                           coords.ctypes.data, *(k[1] for k in keep), pose.ctypes.data, label.ctypes.data, error.ctypes.data,
                           stats.ctypes.data)
    assert rc == 0
    for k, b in zip(keep, before):  # the inputs are only read
        assert b is None or np.array_equal(k[0].view(np.uint8), b.view(np.uint8))
    return pose, label, error, stats


def test_candidates_on_edge_values(host):
    """One candidate at a time: planted triples at several displacements and turns, and the triples that must be skipped."""
    from epipolar_reference import rotation
    rng = np.random.default_rng(0)
    cam = tuple(float(np.float32(v)) for v in (1000.0, 990.0, 960.0, 540.0))
    triples = []
    for i in range(60):
        X = np.stack([rng.uniform(-4, 4, 3), rng.uniform(-2, 2, 3), rng.uniform(3, 12, 3)], axis=1).astype(np.float32).astype(np.float64)
        Rm, t = rotation(*rng.uniform(-0.3, 0.3, 3)), rng.uniform(-1, 1, 3) * (0.3 if i % 2 else 2.0)
        Xc = X @ Rm.T + t
        q = np.rint(16.0 * np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]], axis=1)).astype(np.int64)
        triples.append((X, q))
    X, q = triples[0]
    line = X[0] + np.arange(3)[:, None] * np.array([0.25, 0.5, 0.125])
    triples += [(line, q), (np.stack([X[0], X[0], X[2]]), q), (np.stack([X[0], X[1], X[1]]), q), (X * 0.0, q),
                (np.stack([X[0], X[1], [0.0, 0.0, 0.0]]), q), (X, np.stack([q[0], q[0], q[0]])), (X * 1e-30, q), (X * 1e30, q),
                (X, q * 0 + 2 ** 27), (X[::-1].copy(), q), (-X, q), (X, q[::-1].copy())]
    made = 0
    for X, q in triples:
        Xa, qa = np.ascontiguousarray(X, dtype=np.float64).reshape(9), np.ascontiguousarray(q, dtype=np.int32).reshape(6)
        out = np.full(12, 7.0)
        ok = host.host_p3p_candidate(*cam, Xa.ctypes.data, qa.ctypes.data, out.ctypes.data)
        want = P3.candidate(cam, [[float(v) for v in row] for row in X], [(int(a), int(b)) for a, b in q])
        assert bool(ok) == (want is not None)
        Rw, tw = want if want is not None else P3.EYE
        assert np.array_equal(out.view(np.int64), np.array(list(Rw) + list(tw)).view(np.int64))
        made += ok
    assert 55 <= made <= len(triples) - 5  # the planted ones stand, the degenerate ones are skipped


CASES = {name: (args, kw) for name, args, kw in P3.cases()}
WANT = {}


def want_of(name):
    """The restatement's outputs (and details), computed once and shared."""
    if name not in WANT:
        args, kw = CASES[name]
        details = {}
        WANT[name] = (P3.fit_p3p(*args, details=details, **kw), details)
    return WANT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_bit_for_bit(host, name):
    args, kw = CASES[name]
    want = want_of(name)[0]
    same(run_host(host, *args, **kw), want)
    K = kw["hypotheses"]
    stated_forms(*want, K - 2)  # (stated_forms allows a winner up to its K + 2: here the last candidate is K)
    assert (want[3][..., 2] <= K).all()


def test_cases_cover_what_they_name():
    """The cases reach the branches they are there for (on the restatement, which the two builds equal)."""
    out = {name: want_of(name) for name in CASES if not name.startswith("size_")}
    (po, la, er, st), _ = out["anchor_ring"]
    assert (st[0, :, 2] >= 0).sum() >= 2 and (la[1, :, 7] == -1).all() and (la[0, :, 4] == -1).all()  # released slot, empty slot
    assert (la[0, :, [5, 6, 8, 12 + 2, 12 + 5]] == -1).all() and (la[0, :, [12, 13, 15, 16]] >= 0).any()  # spoiled points, validity bytes
    fitted = st[0, :, 2] >= 0  # a structure point behind the camera: +inf on every fitted row that sees it
    assert np.isinf(er[0, fitted, 10][la[0, fitted, 10] >= 0]).all() and np.isinf(er[0, fitted, 10]).any() and (la[0, :, 10] < 1).all()
    (po, la, er, st), _ = out["fixed_to"]
    assert st[:, 1, 3].tolist() == [32, 32] and st[:, 1, 2].tolist() == [1, 1] and (po[:, 1] == np.eye(3, 4)).all()  # the frame itself
    assert (out["to_ring"][0][3][0, :, 2] >= 0).all() and (out["to_ring"][0][3][0, :, 3] == 0).all()  # a fit on every frame of the ring
    assert (out["valid_all_zero"][0][3] == [0, 0, -1, 0]).all() and (out["valid_all_zero"][0][1] == -1).all()
    (_, _, _, st), det = out["six_points_6"]
    assert st[0, 0].tolist()[:2] == [6, 6] and st[0, 0, 2] >= 0
    counts = det[(0, 0)]["counts"]
    assert counts.count(max(counts)) > 1 and st[0, 0, 2] == counts.index(max(counts))  # ties go to the lowest k
    assert out["six_points_5"][0][3][0, 0].tolist() == [5, 0, -1, 0] and (out["six_points_5"][0][1][0, 0] == [0, 0, 0, -1, 0, 0]).all()
    (_, _, _, st), det = out["degenerate_triples"]
    assert 0 < det[(0, 0)]["made"] < 128 and 0 <= st[0, 0, 2] < 128  # some triples are skipped, a clean one wins
    (_, _, _, st), det = out["all_skipped_2"]
    assert det[(0, 0)]["made"] == 0 and st[0, 0].tolist() == [40, 0, -1, 0]  # nothing but (I, 0) is scored, and it has no fit
    (po, _, _, st), det = out["all_skipped_4000"]
    assert det[(0, 0)]["made"] == 0 and st[0, 0, 2] == 70 and st[0, 0, 0] == 40  # ... and with a wide tolerance it wins
    assert (out["cap_leaves_out"][0][3][0, :, 3] == 23).all() and (out["cap_leaves_out"][0][3][0, :, 2] >= 0).all()
    st = out["lag_wrap_logits"][0][3]
    assert st[0, 0, 2] >= 0 and st[0, 0, 0] > 200
    for K in (63, 64, 65, 255, 256):
        assert out["batch_%d" % K][0][3][0, 0, 2] >= 0
    st = want_of("size_8192_1_33")[0][3]
    assert st[0, 0, 0] == 4096 and st[0, 0, 3] & 8 and st[0, 0, 1] > 4096  # beyond the cap: classified too
    full, over = out["cap_4096"][0], out["cap_4097"][0]
    assert (full[1][0, 0] >= 0).all() and (over[1][0, 0] >= 0).all()  # every slot is a structure point with a correspondence
    assert full[3][0, 0, 0] == 4096 and full[3][0, 0, 3] == 0 and full[3][0, 0, 2] >= 0
    assert over[3][0, 0, 0] == 4096 and over[3][0, 0, 3] == 8 and over[3][0, 0, 2] == full[3][0, 0, 2]
    assert np.array_equal(over[0].view(np.int32), full[0].view(np.int32)) and np.array_equal(over[1][0, 0, :4096], full[1][0, 0])
    assert over[3][0, 0, 1] == full[3][0, 0, 1] + int(over[1][0, 0, 4096] == 1)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/host/p3p_host.cpp as a program with its own main, built with -fsanitize=address,undefined: it runs the same function over
    spoiled inputs in every source form, with 6 to 4200 points (the list cap among them), and must exit clean."""
    exe = str(tmp_path / "p3p_host_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DP3P_HOST_MAIN", "-o", exe, os.path.join(ROOT, "tests", "host", "p3p_host.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert run.returncode == 0, run.stderr[-2000:]
    assert "rows fitted" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


# ---- what the rules are worth: planted scenes through the g++ build -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_hosts(tmp_path_factory):
    """The g++ builds of the three older headers, which equal their numpy restatements bit for bit (their own host tests)."""
    epi, pose, res = (host_library(tmp_path_factory, n) for n in ("epipolar", "pose", "resection"))
    epi.host_fit_epipolar.restype = C.c_int
    epi.host_fit_epipolar.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 5 + [C.c_void_p] * 12
    pose.host_fit_pose.restype = C.c_int
    pose.host_fit_pose.argtypes = [C.c_int] * 10 + [C.c_float] * 7 + [C.c_void_p] * 13
    res.host_fit_resection.restype = C.c_int
    res.host_fit_resection.argtypes = [C.c_int] * 11 + [C.c_uint32] + [C.c_float] * 8 + [C.c_void_p] * 14
    return epi, pose, res


def rms(a):
    return float(np.sqrt((np.asarray(a) ** 2).mean()))


def against_the_reference(po, la, truth, X, q, static, frames):
    """Poses and labels of `frames` rows against the planted poses: the 1 % cap on dropped static points (the float64 reference,
    reference_pose over the entries labelled 1 started at the planted pose, is held to the cap first) -> (position RMS, rotation RMS,
    the reference's two, the largest differences to the reference: position, rotation in degrees)."""
    pairs = dropped = ref_dropped = 0
    pos, pos_f, rot, rot_f, diff_pos, diff_rot = [], [], [], [], 0.0, 0.0
    for j in frames:
        Rt, tt = truth[j, :, :3], truth[j, :, 3]
        Rm, t = po[j, :, :3].astype(np.float64), po[j, :, 3].astype(np.float64)
        kept = la[j] == 1
        Rf, tf = reference_pose(Rt.copy(), tt.copy(), X[kept], q[j][kept])
        within = reprojection(Rt, tt, X[static], q[j][static]) <= 4.0
        pairs += int(within.sum())
        dropped += int((within & (la[j][static] == 0)).sum())
        ref_dropped += int((within & ~(reprojection(Rf, tf, X[static], q[j][static]) <= 4.0)).sum())
        pos.append(np.linalg.norm(centre(Rm, t) - centre(Rt, tt))), pos_f.append(np.linalg.norm(centre(Rf, tf) - centre(Rt, tt)))
        rot.append(rotation_angle(Rm, Rt)), rot_f.append(rotation_angle(Rf, Rt))
        diff_pos, diff_rot = max(diff_pos, float(np.linalg.norm(centre(Rm, t) - centre(Rf, tf)))), max(diff_rot, rotation_angle(Rm, Rf))
    assert ref_dropped <= 0.01 * pairs, (ref_dropped, pairs)  # the reference itself stays inside the cap on these inputs
    assert dropped <= 0.01 * pairs, (dropped, pairs)
    return rms(pos), rms(rot), rms(pos_f), rms(rot_f), diff_pos, diff_rot


@pytest.mark.parametrize("kind", KINDS)
def test_planted_paths(host, chain_hosts, kind):
    """test_resection_host.test_planted_paths with ctk_fit_p3p's rules in place of the three-step chain: the same scenes
    (resection_reference.planted_path: 1080p, focal length 1000 px, depths 3..12 m, 0.1 px noise, 25 % movers in three groups;
    sideways, forward, 90 points; a path of 12 frames, 20 seeds each), the same planted reconstruct through the g++ builds of
    epipolar_math.h and pose_math.h, then per frame ONE call of the g++ build of p3p_math.h (256 hypotheses, tol 2, min_points 16).

    Conditions, as there: the structure's own frame gives exactly (I | 0); every frame has a fit and no round falls back; no static
    structure point that lies within tol under the planted pose is labelled 0 on more than 1 % of the (frame, point) pairs (the
    float64 reference is held to the cap first); every mover that is kept has an error <= tol^2.  Bounds: per scene, the RMS over the
    11 other frames of the camera-position error and of the rotation error against the planted path are within 1.10 x the float64
    reference's (both fit the same inliers; they differ by three rounds against convergence and by float32 outputs: the same
    allowance for the same reason).

    Measured, worst of 20 seeds (rules / reference RMS ratio: position, rotation; largest difference to the reference over all
    frames: position in baselines, rotation in degrees):
      sideways  1.0000005  1.0000051   1.6e-05  2.0e-06
      forward   1.0000019  1.0000047   2.8e-05  2.0e-06
      few       1.0000004  1.0000027   1.8e-07  1.9e-06"""
    from test_epipolar_host import run_host as run_epipolar
    from test_pose_host import run_host as run_pose
    epi_host, pose_host, _ = chain_hosts
    worst_pos, worst_rot, diff_pos, diff_rot = 0.0, 0.0, 0.0, 0.0
    for seed in range(20):
        sc = RR.planted_path(seed, kind, T)
        coords, mover = sc["coords"], sc["mover"]
        N = coords.shape[2]
        visible = np.ones((1, T + 2, N), dtype=np.uint8)
        two_view = dict(K=512, tol=1.0, min_points=16, min_base=16.0, seed=0)
        fu, lab, _, est = run_epipolar(epi_host, coords, visible=visible, f0=1, F=1, lag=1, **two_view)
        assert est[0, 0, 2] >= 0
        _, de, _ = run_pose(pose_host, coords, CAM, fu, lab, visible=visible, f0=1, F=1, lag=1, min_points=16)
        pts, valid = RR.structure_from_pose(coords[0, 1], CAM, de[0, 0], lab[0, 0])
        src = dict(visible=visible, f0=2, F=T, anchor=(coords[:, 1].copy(), visible[:, 1].copy(), 1))
        po, la, er, st = run_host(host, coords, CAM, pts[None], valid[None], tol=2.0, hypotheses=256, seed=0, min_points=16, **src)
        assert np.array_equal(po[0, 0], np.eye(3, 4, dtype=np.float32)) and st[0, 0, 3] == 32  # the structure's own frame: exactly (I | 0)
        assert (st[0, :, 2] >= 0).all() and (st[0, 1:, 3] == 0).all(), (seed, st[0])
        kept = la[0] == 1
        assert (er[0][kept] <= 4.0).all() and (er[0][kept & mover[None]] <= 4.0).all()  # every mover that is kept lies within tol
        ok, q16 = R.quant(coords[0], 1.0)
        assert ok.all()
        static = (valid == 1) & ~mover
        pos, rot, pos_f, rot_f, dp, dr = against_the_reference(po[0], la[0], sc["truth"], pts.astype(np.float64), (q16 / 16.0)[2:], static,
                                                               range(1, T))
        assert pos <= 1.10 * pos_f and rot <= 1.10 * rot_f, (seed, pos, pos_f, rot, rot_f)
        worst_pos, worst_rot, diff_pos, diff_rot = max(worst_pos, pos / pos_f), max(worst_rot, rot / rot_f), max(diff_pos, dp), max(diff_rot, dr)
    print(kind, "rules / reference RMS ratio: position", worst_pos, "rotation", worst_rot, "; largest difference to the reference:",
          diff_pos, "baselines,", diff_rot, "deg")


def chain_finds(chain_hosts, coords, pts, valid, truth):
    """The three older rules chained as localize() chains them (512 / 256 hypotheses, tol 1 / 2) -> on how many of the frames the pose
    lies within 0.2 degrees and 0.05 units of the planted one."""
    from test_epipolar_host import run_host as run_epipolar
    from test_pose_host import run_host as run_pose
    from test_resection_host import run_host as run_resection
    epi_host, pose_host, res_host = chain_hosts
    n = coords.shape[1] - 1
    visible = np.ones(coords.shape[:3], dtype=np.uint8)
    src = dict(visible=visible, f0=1, F=n, to=0)
    fu, lab, _, _ = run_epipolar(epi_host, coords, mask=valid[None], K=512, tol=1.0, min_points=16, min_base=16.0, seed=0, **src)
    seeds, _, _ = run_pose(pose_host, coords, CAM, fu, lab, mask=valid[None], min_points=16, **src)
    po, _, _, st = run_resection(res_host, coords, CAM, pts[None], valid[None], seeds, tol=2.0, hypotheses=256, seed=0, min_points=16, **src)
    return sum(found(po[0, j], st[0, j], truth[j]) for j in range(n))


def found(po, st, truth):
    Rm, t = po[:, :3].astype(np.float64), po[:, 3].astype(np.float64)
    return bool(st[2] >= 0 and rotation_angle(Rm, truth[:, :3]) <= 0.2 and np.linalg.norm(centre(Rm, t) - centre(truth[:, :3], truth[:, 3])) <= 0.05)


def planted_scenes(host, chain_hosts, scenes):
    """scenes: (seed, dict of p3p_reference.contaminated) one after the other -> the conditions held on every one; the measured
    (frames, frames the chain finds, frames these rules find, worst RMS ratios, largest differences to the reference)."""
    frames = chain = mine = 0
    worst_pos, worst_rot, diff_pos, diff_rot = 0.0, 0.0, 0.0, 0.0
    for seed, sc in scenes:
        coords, mover, pts = sc["coords"], sc["mover"], sc["structure"]
        n, N = coords.shape[1] - 1, coords.shape[2]
        valid = np.ones(N, dtype=np.int8)
        visible = np.ones((1, n + 1, N), dtype=np.uint8)
        po, la, er, st = run_host(host, coords, CAM, pts[None], valid[None], visible=visible, f0=1, F=n, to=0, tol=2.0, hypotheses=256,
                                  seed=0, min_points=16)
        assert (st[0, :, 2] >= 0).all() and (st[0, :, 3] == 0).all(), (seed, st[0])  # every frame has a fit, no round falls back
        kept = la[0] == 1
        assert (er[0][kept & mover[None]] <= 4.0).all()  # every mover that is kept lies within tol
        ok, q16 = R.quant(coords[0], 1.0)
        assert ok.all()
        pos, rot, pos_f, rot_f, dp, dr = against_the_reference(po[0], la[0], sc["truth"], pts.astype(np.float64), (q16 / 16.0)[1:], ~mover,
                                                               range(n))
        assert pos <= 1.10 * pos_f and rot <= 1.10 * rot_f, (seed, pos, pos_f, rot, rot_f)
        worst_pos, worst_rot, diff_pos, diff_rot = max(worst_pos, pos / pos_f), max(worst_rot, rot / rot_f), max(diff_pos, dp), max(diff_rot, dr)
        frames += n
        chain += chain_finds(chain_hosts, coords, pts, valid, sc["truth"])
        mine += sum(found(po[0, j], st[0, j], sc["truth"][j]) for j in range(n))
    return frames, chain, mine, worst_pos, worst_rot, diff_pos, diff_rot


@pytest.mark.parametrize("share", (0.6, 0.7))
def test_contaminated_structure(host, chain_hosts, share):
    """The scenes the entry point is for (p3p_reference.contaminated): 1080p, focal length 1000 px, 400 points 3..12 deep, 0.1 px noise,
    the camera 0.2..0.6 units sideways with up to +-0.02 rad of turn, the structure the truth with 0.3 % depth noise and every point
    valid; 60 % and 70 % of the points move individually by 8..60 px on every frame; 20 seeds x three frames, through the g++ build
    (256 hypotheses, tol 2, min_points 16).

    Conditions: every frame has a fit and no round falls back; every mover that is kept has an error <= tol^2; no static point that
    lies within tol under the planted pose is labelled 0 on more than 1 % of the (frame, point) pairs (the float64 reference is held
    to the cap first); per scene the RMS of the camera-position error and of the rotation error are within 1.10 x the float64
    reference's.

    Measured over the 60 frames of a share (frames these rules bring within 0.2 degrees and 0.05 units of the planted pose; frames
    the chain of the three older rules does, run as localize() runs them with 512 / 256 hypotheses and tol 1 / 2 through their g++
    builds, which equal the numpy references bit for bit -- a record, not an assertion; worst rules / reference RMS ratio: position,
    rotation; largest difference to the reference: position in units, rotation in degrees):
      60 %  these rules 60 of 60, the chain 54 of 60   1.000027  1.000012   3.4e-08  1.7e-06
      70 %  these rules 60 of 60, the chain 14 of 60   1.000034  1.000008   4.6e-08  2.0e-06"""
    out = planted_scenes(host, chain_hosts, ((seed, P3.contaminated(seed, share)) for seed in range(20)))
    print("share", share, "frames", out[0], "chain finds", out[1], "p3p finds", out[2], "RMS ratios", out[3], out[4], "differences", out[5], out[6])
    assert out[2] == out[0]


@pytest.mark.parametrize("N", (400, 40))
def test_planar_structure(host, chain_hosts, N):
    """A structure on ONE slanted plane (0.45 X - 0.25 Y + Z = 6, depths about 4.5..9), on which the eight-point fit of the chain has no
    unique matrix: p3p_reference.contaminated(plane=True) with 25 % movers, 400 and 40 points, 20 seeds x three frames.  The same
    conditions as test_contaminated_structure.

    Measured over the 60 frames of a size (as there):
      400 points  these rules 60 of 60, the chain 33 of 60   1.000017  1.000006   3.7e-08  1.7e-06
      40 points   these rules 60 of 60, the chain  1 of 60   1.000013  1.000002   3.6e-08  1.8e-06"""
    out = planted_scenes(host, chain_hosts, ((seed, P3.contaminated(seed, 0.25, N=N, plane=True)) for seed in range(20)))
    print("plane N", N, "frames", out[0], "chain finds", out[1], "p3p finds", out[2], "RMS ratios", out[3], out[4], "differences", out[5], out[6])
    assert out[2] == out[0]
