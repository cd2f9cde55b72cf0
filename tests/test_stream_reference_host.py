"""tests/stream_reference.py checked without a GPU, over the case list of tests/test_gpu_stream_matrix.py:
  - against the torch expressions of the reference's streaming glue evaluated on the CPU (the carry-over and write-back that
    tests/test_gpu_stream_groups.py writes out, the index expressions of the assign tests), bit for bit;
  - the case list reaches every branch the matrix names;
  - every logit pair that emit or health thresholds is decisive or at least MARGIN from the threshold."""
import numpy as np
import torch

import stream_reference as ref
import test_gpu_stream_matrix as M
from stream_reference import BIG, EMPTY_FRAME, LEVELS, f32


def words(a):
    a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
    return M._words(a)


def frames_long(q0):
    """torch's .long() where the rule leaves the frame alone, the frame of no window elsewhere."""
    ok = (q0 >= -2.0 ** 31) & (q0 < 2.0 ** 31)
    return torch.where(ok, torch.where(ok, q0, torch.zeros_like(q0)).long(), torch.full(q0.shape, ref.NO_FRAME, dtype=torch.int64))


def over_stride(x, stride):
    """x / stride as the reference's glue evaluates it where it runs, on the GPU: torch divides a tensor by a host scalar there as a
    multiplication with the scalar's float32 reciprocal.  For a power of two that is the division the CPU performs, and the
    expression is left as written; for any other stride the CPU would divide, so the multiplication is spelled out."""
    return x / stride if float(stride).hex().startswith("0x1.0000000000000p") else x * (1.0 / stride)


def test_qframe_rule():
    q = np.array([0.0, -0.5, 0.99, -1.0, -1.5, 7.75, 2.0 ** 30, -2.0 ** 31, 2.0 ** 31, np.nan, np.inf, -np.inf, 1e30, -1e30,
                  np.nextafter(f32(2.0 ** 31), f32(0)), np.nextafter(f32(-2.0 ** 31), f32(-np.inf))], f32)
    n = ref.NO_FRAME
    assert ref.qframe(q).tolist() == [0, 0, 0, -1, -1, 7, 2 ** 30, -2 ** 31, n, n, n, n, n, n, 2 ** 31 - 128, n]
    assert ref.NO_FRAME > 2 ** 31 + 2 ** 30  # beyond every ind + S the entry points admit
    assert ref.row_of(37, 13, True) == 11 and ref.row_of(37, 13, False) == 37 and ref.row_of(2 ** 30 - 64, 67, True) == (2 ** 30 - 64) % 67


def test_begin_is_the_torch_carry_over():
    for c in M.BEGIN:
        st = M.state_begin(c)
        want = M.want_begin(c, st)
        G, N, S, step, ind, ov = c.G, c.N, c.S, c.step, c.ind, c.overlap
        q = torch.from_numpy(st["queries"].reshape(G, N, 3))
        hc, hv, hf = (torch.from_numpy(st[k]) for k in ("hc", "hv", "hf"))
        rows = [ref.row_of(ind + t, c.R, c.ring) for t in range(ov)]
        for b in range(G):
            qframes, qcoords = frames_long(q[b, :, 0]), over_stride(q[b, :, 1:3], c.stride).contiguous()
            coords = qcoords[None].expand(S, N, 2).contiguous()
            vis, conf = torch.zeros(S, N), torch.zeros(S, N)
            if ind > 0:  # CoTrackerThreeOnline._video_gen
                copy_over = (qframes < ind + ov)[None, :]
                cprev = over_stride(hc[b, rows], c.stride)
                cprev = torch.cat([cprev, cprev[-1:].expand(step, -1, -1)], dim=0)
                vprev = torch.cat([hv[b, rows], hv[b, rows][-1:].expand(step, -1)], dim=0)
                fprev = torch.cat([hf[b, rows], hf[b, rows][-1:].expand(step, -1)], dim=0)
                coords = torch.where(copy_over[..., None], cprev, coords)
                vis, conf = torch.where(copy_over, vprev, vis), torch.where(copy_over, fprev, conf)
            mask = (qframes < ind + S).to(torch.uint8)
            for name, got in (("coords", coords), ("vis", vis), ("conf", conf)):
                assert np.array_equal(words(got), words(want[name][b])), (c.id, b, name)
            assert np.array_equal(mask.numpy(), want["mask"].reshape(G, N)[b]), (c.id, b)


def test_commit_is_the_torch_write_back():
    runs = [(c, None) for c in M.COMMIT] + [(c, plant) for c, _, plant in M.FLAG_RUNS]
    for c, plant in runs:
        st = M.state_commit(c, plant, flag=6 if plant else 0)
        want = M.want_commit(c, st)
        T = c.T_valid
        coords, vis, conf, hc, hv, hf = (torch.from_numpy(st[k].copy()) for k in ("coords", "vis", "conf", "hc", "hv", "hf"))
        rows = [ref.row_of(c.ind + t, c.R, c.ring) for t in range(T)]
        new = (coords[:, :T] * float(c.stride), vis[:, :T], conf[:, :T])
        for h_, v in zip((hc, hv, hf), new):
            h_[:, rows] = v
        finite = all(bool(torch.isfinite(v).all()) for v in new)
        for name, got in (("hc", hc), ("hv", hv), ("hf", hf)):
            assert np.array_equal(words(got), words(want[name])), (c.id, name)
        assert int(want["flag"][0]) == (6 if plant else 0) | (not finite), c.id
        assert (plant is None) == finite


def test_assign_is_the_index_expressions():
    for c in M.ASSIGN:
        st = M.state_assign(c)
        want = M.want_assign(c, st)
        P = c.G * c.N
        slots = torch.from_numpy(st["slots"]).long()
        ok = (slots >= 0) & (slots < P)
        sd = slots[ok]
        queries = torch.from_numpy(st["queries"].copy()).view(torch.int32).view(P, 3)  # (moved as integers: random bytes)
        queries[sd] = torch.from_numpy(st["newq"]).view(torch.int32).view(-1, 3)[ok]
        assert np.array_equal(words(queries), words(want["queries"])), c.id
        nrows = c.R if c.ring else c.get("rows")
        for l in range(LEVELS):
            acc = torch.from_numpy(st[f"acc{l}"].copy())
            acc[sd] = 0.0
            assert np.array_equal(words(acc), words(want[f"acc{l}"])), (c.id, l)
        for k in ("hc", "hv", "hf"):
            h_ = torch.from_numpy(st[k].copy())
            h_[sd // c.N, :nrows, sd % c.N] = 0.0
            assert np.array_equal(words(h_), words(want[k])), (c.id, k)
        assert len(set(st["slots"].tolist())) == len(st["slots"]) <= P


def test_resident_assign_is_the_plain_assign_plus_patch_and_carry_rows():
    """Against the index expressions of tests/test_gpu_stream_resident.py, the patch from the shared sampler restatement."""
    for c in M.RESIDENT:
        st = M.state_assign(c)
        want = M.want_assign(c, st)
        plain = M.want_assign(c, st, plain=True)
        Mn = len(st["slots"])
        newq = st["newq"].reshape(Mn, 3)
        qf = ref.qframe(newq[:, 0])
        res = (qf >= c.ind - c.step) & (qf < c.ind + c.overlap) & (st["slots"] >= 0) & (st["slots"] < c.G * c.N)
        carry = [ref.row_of(f, c.R, c.ring) for f in range(c.ind, c.ind + c.overlap)]
        for m in np.nonzero(res)[0]:
            g, n = divmod(int(st["slots"][m]), c.N)
            for r in carry:
                plain["hc"][g, r, n], plain["hv"][g, r, n], plain["hf"][g, r, n] = newq[m, 1:], 0.0, 0.0
            for l in range(LEVELS):
                xy = ref.level_xy(newq[m:m + 1, 1:], c.stride, l)
                plain[f"acc{l}"][int(st["slots"][m])] = f32(0.0) + ref.patch(st[f"fm{l}"], [qf[m] - (c.ind - c.step)], xy)[0]
        for k in want:
            assert np.array_equal(words(plain[k]), words(want[k])), (c.id, k)
        if not c.ring and c.get("rows") < c.ind:  # the rows between the cleared ones and the carry rows keep their bytes
            for k in ("hc", "hv", "hf"):
                assert np.array_equal(words(want[k][:, c.get("rows"):c.ind]), words(st[k][:, c.get("rows"):c.ind])), c.id


def test_support_adds_the_patch_of_the_sampled_points_only():
    for c in M.SUPPORT:
        st = M.state_support(c)
        want = M.want_support(c, st)
        q = st["queries"].reshape(-1, 3)
        qf = ref.qframe(q[:, 0])
        left, right = (0 if c.ind == 0 else c.ind + c.step), c.ind + c.S
        hit = (qf >= left) & (qf < right)
        assert hit.any(), c.id
        for l in range(LEVELS):
            a, b = st[f"acc{l}"], want[f"acc{l}"]
            assert np.array_equal(words(a[~hit]), words(b[~hit])), (c.id, l)
            assert np.isfinite(b[hit]).all() and (a[hit] != b[hit]).any(), (c.id, l)
        gone = np.isnan(q[:, 0]) | np.isin(q[:, 0], np.array(M.NO_WINDOW, f32))
        assert not (hit & gone).any()  # a frame of no window is never sampled
        if c.ind == 0 and (q[:, 0] == f32(-0.5)).any():
            assert hit[q[:, 0] == f32(-0.5)].all()  # -0.5 truncates to frame 0: sampled in the first window


def test_case_list_covers_every_axis():
    shapes = {(8, 4), (16, 8), (8, 3), (8, 7), (8, 1), (2, 1)}
    for cases in (M.BEGIN, M.COMMIT):
        assert {c.N for c in cases} >= {1, 63, 64, 65, 255, 256, 257, 513} and {c.G for c in cases} == {1, 3}
        assert {(c.S, c.step) for c in cases} >= shapes | {(64, 32)}
        lin = [c for c in cases if not c.ring]
        ring = [c for c in cases if c.ring]
        assert {c.N for c in lin} >= {1, 63, 64, 65, 255, 256, 257, 513} and {c.N for c in ring} >= {1, 63, 64, 65, 255, 256, 257, 513}
        assert any(c.ind == 0 for c in lin) and any(c.ind == c.step for c in lin) and any(c.ind > c.step for c in lin)
        assert any((c.G * c.S * c.N) % 256 and 256 % c.N and c.G * c.S * c.N > 256 for c in lin)  # a partly live last block, blocks astride (g, t)
        assert all(c.R >= c.ind + c.S for c in lin) and all(c.R >= c.S for c in ring)
        assert {"S", "S+1", "13", "2S"} <= {k for c in ring for k, r in (("S", c.S), ("S+1", c.S + 1), ("13", 13), ("2S", 2 * c.S)) if c.R == r}
        assert any(c.ind == M.LIMIT and c.S == 64 and c.step == 32 for c in ring) and any(c.ind == 0 for c in ring)
        assert any(c.overlap == 1 for c in cases) and any(c.overlap == c.S - 1 and c.S == 8 for c in cases)
    assert {(M.carry_wraps(c), M.commit_wraps(c)) for c in M.COMMIT} == {(False, False), (True, False), (False, True), (True, True)}
    assert [(c.ring, c.S, c.step, c.ind, c.R) for c in M.BEGIN] == [(c.ring, c.S, c.step, c.ind, c.R) for c in M.COMMIT]  # one call's begin and commit
    for c in M.COMMIT:
        assert c.T_valid in (1, c.S - 1, c.S)
    assert {("1" if c.T_valid == 1 else "S" if c.T_valid == c.S else "S-1") for c in M.COMMIT if c.S > 2} == {"1", "S-1", "S"}
    # query frames: every begin case with enough points holds every frame of the list; the limit case its two pinned frames
    for c in M.BEGIN:
        q0 = M.state_begin(c)["queries"].reshape(-1, 3)[:, 0]
        if c.ind == M.LIMIT:
            assert q0[0] == EMPTY_FRAME == c.ind + c.S and q0[1] == c.ind + c.S - 64
        elif c.G * c.N >= 32:
            fl = np.array(M.frame_list(c), f32)
            assert all((np.isnan(q0).any() if np.isnan(f) else (q0 == f).any()) for f in fl), c.id
    fl = M.frame_list(M.BEGIN[1])
    c = M.BEGIN[1]
    assert {c.ind + c.step - 1, c.ind + c.step, c.ind + c.S - 1, c.ind + c.S, c.ind + c.overlap - 1, c.ind + c.overlap, -0.5, -3.0,
            float(EMPTY_FRAME), np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31} <= set(fl) and any(np.isnan(f) for f in fl)
    # commit flag: every place the matrix names, every tensor, every value
    labels = {label.split("-x-")[0].split("-y-")[0].split("-v-")[0].split("-c-")[0] for _, label, _ in M.FLAG_RUNS}
    assert labels >= {"lane0", "lane63", "wave3", "last-live", "only-live-of-block1", "lane1-of-block1", "lane0-wave1-block1"}
    assert {(p[0], p[1][3:], str(p[2])) for _, _, p in M.FLAG_RUNS} == {(n, k, v) for n, k in (("coords", (0,)), ("coords", (1,)), ("vis", ()), ("conf", ()))
                                                                        for v in ("nan", "inf", "-inf")}
    for c, places in M.FLAG:
        for label, th in places.items():
            n = th if c.ring else th % c.N
            assert n < c.N and (c.ring or th < c.G * c.T_valid * c.N), (c.id, label)
            lane, wave, block = th % 64, (th % 256) // 64, th // 256
            want = {"lane0": lane == 0, "lane63": lane == 63, "wave3": wave == 3, "wave3-block1": wave == 3 and block == 1,
                    "last-live": th == (c.N if c.ring else c.G * c.T_valid * c.N) - 1, "only-live-of-block1": block == 1 and c.N == th + 1 == 257,
                    "lane1-of-block1": block == 1 and lane == 1 and wave == 0, "lane0-wave1-block1": block == 1 and wave == 1 and lane == 0}
            assert want[label], (c.id, label)
    assert {c.N for c, _ in M.FLAG if c.ring} >= {257, 258, 321}
    # support and the assigns
    for cases in (M.SUPPORT, M.ASSIGN, M.RESIDENT):
        assert all(c.G * c.N <= 320 for c in cases)
    assert {c.G * c.N for c in M.SUPPORT} >= {1, 2, 3, 4, 67} and {(c.G * c.N * 49) % 4 for c in M.SUPPORT} == {0, 1, 2, 3}
    assert {c.pyr for c in M.SUPPORT} == {"model", "odd", "ones"} == set(M.PYRAMIDS) and any(c.ring for c in M.SUPPORT)
    seen = set()
    for c in M.SUPPORT:
        q = M.state_support(c)["queries"].reshape(-1, 3)
        qf = ref.qframe(q[:, 0])
        hit = (qf >= (0 if c.ind == 0 else c.ind + c.step)) & (qf < c.ind + c.S)
        for x, y in q[hit, 1:]:
            tags = {"nan": np.isnan(x) or np.isnan(y), "+inf": x == np.inf or y == np.inf, "-inf": x == -np.inf or y == -np.inf,
                    "1e30": x == f32(1e30), "half": x == 12.5, "integer": x == 40.0, "corner": x == 0.0 and y == 0.0,
                    "outside": x == f32(-8 * c.stride), "interior": x == f32(33.3)}
            seen |= {k for k, v in tags.items() if v}
    assert seen == {"nan", "+inf", "-inf", "1e30", "half", "integer", "corner", "outside", "interior"}
    for cases in (M.ASSIGN, M.RESIDENT):
        assert {c.get("M") for c in cases} >= {"one", "all", "list", "list+out"} and any(c.ring for c in cases) and any(not c.ring for c in cases)
    assert {"0", "1", "T_cap", "between"} <= {k for c in M.ASSIGN if not c.ring for k, ok in (("0", c.get("rows") == 0), ("1", c.get("rows") == 1),
                                                                                              ("T_cap", c.get("rows") == c.R), ("between", 1 < c.get("rows") < c.R)) if ok}
    for c in M.ASSIGN + M.RESIDENT:
        s = M.state_assign(c)["slots"]
        if c.get("M").startswith("list"):
            assert {g * c.N for g in range(c.G)} | {g * c.N + c.N - 1 for g in range(c.G)} <= set(s.tolist()), c.id
            assert sorted(s.tolist()) != s.tolist()
        if c.get("M") == "list+out":
            assert {-1, c.G * c.N, BIG} <= set(s.tolist())
    assert {(c.S, c.step) for c in M.RESIDENT} >= {(8, 4), (16, 8)}
    assert any(c.ring and (c.ind % c.R) + c.overlap > c.R and (c.S, c.step) == sh for c in M.RESIDENT for sh in [(8, 4)])
    assert any(c.ring and (c.ind % c.R) + c.overlap > c.R and (c.S, c.step) == (16, 8) for c in M.RESIDENT)
    assert any(not c.ring and 0 < c.get("rows") < c.ind for c in M.RESIDENT) and any(c.get("frames") == "outside" for c in M.RESIDENT)
    assert any(c.ring and c.R == c.S for c in M.RESIDENT)
    c = M.RESIDENT[0]
    newq = M.state_assign(c)["newq"].reshape(-1, 3)
    qf = ref.qframe(newq[:17, 0])
    assert ((qf >= c.ind - c.step) & (qf < c.ind + c.overlap)).tolist() == [True] * 6 + [False] * 9 + [True] * 2
    # emit
    assert {("N" if c.get("No") == c.N else "N-1" if c.get("No") == c.N - 1 else str(c.get("No"))) for c in M.EMIT} >= {"N", "N-1", "1", "256", "257"}
    assert {c.N for c in M.EMIT} >= {1, 63, 64, 65, 255, 256, 257, 513} and {c.G for c in M.EMIT} == {1, 3}
    assert any(c.get("f1") - c.get("f0") == c.R for c in M.EMIT) and any(c.get("f0") % c.R + c.get("f1") - c.get("f0") > c.R for c in M.EMIT)
    assert {c.get("absent") for c in M.EMIT} >= {(), ("vis_logit",), ("conf_logit",), ("visible",)} and any(not c.get("first") for c in M.EMIT)
    assert any(c.get("f1") == 2 ** 30 for c in M.EMIT) and all(c.ring or c.R >= c.get("f1") for c in M.EMIT)
    assert all((M.state_emit(c)["first_row"] == BIG).any() for c in M.EMIT if c.G * c.N > 60)
    # health
    grids = {(c.get("grid"), c.get("No")) for c in M.HEALTH}
    assert {((1, 1), 513), ((1, 2), 513)} <= grids and any(g[0] * g[1] == 4096 and no == 1 for g, no in grids)
    assert any((g[0] * g[1]) % ((no + 255) // 256) for g, no in grids) and all(c.ring or c.R >= c.get("f1") for c in M.HEALTH)
    for c in M.HEALTH:
        st = M.state_health(c)
        lost = M.want_health(c, st)[0]["lost"]
        if c.get("No") > 100:
            assert set(lost.reshape(-1).tolist()) >= {-1, 0, 1}, c.id


def test_visibility_margin():
    """Every logit pair emit or health can threshold: the float64 product is decisive (a NaN; an infinity or +-88 / +-104, where expf
    saturates and the product is 0, the other sigmoid or NaN) or at least MARGIN from the threshold.  All of them are at least MARGIN
    away or NaN, the decisive ones included, so no entry is left out of any comparison."""
    t = np.float64(f32(M.THRESH))
    n = 0
    for c in M.EMIT + M.HEALTH:
        st = (M.state_emit if c.kernel == "emit" else M.state_health)(c)
        p = ref.visible_product(st["hv"], st["hf"])  # every pair of the history, read or not
        assert (np.isnan(p) | (np.abs(p - t) >= M.MARGIN)).all(), c.id
        assert (np.isnan(p) == (np.isnan(st["hv"]) | np.isnan(st["hf"]))).all()
        _, pr = (M.want_emit if c.kernel == "emit" else M.want_health)(c, st)
        assert (np.isnan(pr) | (np.abs(pr - t) >= M.MARGIN)).all(), c.id
        if p.size > 2000:
            assert (p > t).any() and (p < t).any() and np.isnan(p).any()
        n += p.size
    assert n > 10000
