"""Track health and replenish, the part that needs no GPU: ctk_stream_health is declared, bound and exported without an ABI bump, the
new struct's ctypes mirror has the compiler's layout, every refusal comes back before any launch, the policy function
choose_replenish does what CoTrackerOnlinePredictor.replenish documents, and the model and predictor refuse what they must."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from ctk_support import ROOT, header_layout, lib  # noqa: F401

E_NULL, E_SHAPE = -1, -2
POINTERS = ("queries", "hist_coords", "hist_vis", "hist_conf", "first_row", "lost", "cell", "cover")


def test_declared_bound_exported_and_abi(lib):
    from cotracker_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ctk.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = "ctk_stream_health"
    assert re.search(r"\bint %s\(" % name, header)
    assert name in L.SYMBOLS and hasattr(lib, name)
    assert any(ln.split()[-1] == name and " T " in ln for ln in nm.splitlines())
    assert lib.ctk_abi_version() == L.ABI_VERSION == 9  # additive
    assert int(header_layout()["sizeof"]["ctk_stream_args"]) == C.sizeof(L.StreamArgs) == 200  # the struct did not grow
    assert name in header.split("#define CTK_ABI_VERSION")[0]  # the ABI history names the addition


def test_health_args_mirror_matches_the_compiler():
    """sizeof and every offsetof of ctk_stream_health_args, from a C program compiled against include/ctk.h."""
    from cotracker_amd import _lib as L
    fields = [f[0] for f in L.StreamHealth.Args._fields_]
    lines = ['printf("S %zu\\n", sizeof(ctk_stream_health_args));']
    lines += [f'printf("F {f} %zu\\n", offsetof(ctk_stream_health_args, {f}));' for f in fields]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "health_layout.c"), os.path.join(d, "health_layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "ctk.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(out[0].split()[1]) == C.sizeof(L.StreamHealth.Args)
    got = {ln.split()[1]: int(ln.split()[2]) for ln in out[1:]}
    assert got == {f: getattr(L.StreamHealth.Args, f).offset for f in fields}
    assert len(got) == 25
    # the header declares the fields in the mirror's order and no others
    body = re.search(r"typedef struct ctk_stream_health_args \{(.*?)\} ctk_stream_health_args;", open(os.path.join(ROOT, "include", "ctk.h")).read(),
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == fields


def health_args(**kw):
    """A ctk_stream_health_args that passes every check: a ring of 16 rows far into a stream, an 8 x 12 grid over a 64 x 96 picture."""
    from cotracker_amd import _lib as L
    a = L.StreamHealth.Args()
    a.G, a.N, a.N_out, a.R, a.f1, a.look, a.ind_next = 3, 10, 7, 16, 1016, 8, 1012
    a.thresh, a.x_lo, a.x_hi, a.y_lo, a.y_hi, a.gh, a.gw, a.inv_cw, a.inv_ch, a.reserved = 0.6, 0.0, 95.0, 0.0, 63.0, 8, 12, 12 / 95, 8 / 63, 0
    for n in POINTERS:
        setattr(a, n, 4096)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_health_refuses_before_any_launch(lib):
    """Every refusal is an E_* code (a launch on a machine without a GPU would be a hipError_t > 0)."""
    health = lambda a: lib.ctk_stream_health(None if a is None else C.byref(a), None)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    assert health(None) == E_NULL
    for f in POINTERS:
        assert health(health_args(**{f: None})) == E_NULL, f
    for field, values in (("G", (0, -1, 65536)), ("N", (0, -1, 2 ** 30)), ("N_out", (0, -1, 11)), ("R", (0, -1, 7)), ("gh", (0, -1, 342)),
                          ("gw", (0, -1, 513)), ("f1", (0, -1, 7, 2 ** 30 + 1)), ("look", (0, -1, 17, 1017)), ("ind_next", (-1, -4)),
                          ("thresh", (nan,)), ("x_lo", (nan, inf, -inf, 95.0, 96.0)), ("x_hi", (nan, inf, -inf, 0.0, -1.0)),
                          ("y_lo", (nan, inf, -inf, 63.0, 64.0)), ("y_hi", (nan, inf, -inf, 0.0, -1.0)), ("inv_cw", (nan, inf, 0.0, -0.1)),
                          ("inv_ch", (nan, inf, 0.0, -0.1)), ("reserved", (1, -1))):
        for v in values:
            assert health(health_args(**{field: v})) == E_SHAPE, (field, v)
    assert health(health_args(gh=64, gw=65)) == E_SHAPE  # 4160 cells
    assert health(health_args(R=2000, look=1017)) == E_SHAPE  # look > f1
    assert health(health_args(G=8, N=2 ** 23 + 1, N_out=1)) == E_SHAPE  # G * N > 2^26
    # what the rules admit reaches the pointer check: the refusal is then the NULL one
    for kw in (dict(gh=64, gw=64), dict(look=16), dict(look=1), dict(R=2 ** 30, f1=2 ** 30, look=2 ** 30), dict(G=65535, N=1, N_out=1),
               dict(ind_next=0), dict(thresh=inf), dict(thresh=-1.0), dict(N_out=10)):
        assert health(health_args(cover=None, **kw)) == E_NULL, kw


# ---- the policy -----------------------------------------------------------------------------------------------------------------
def choose(lost, cover, occupied, max_lost, max_new=None):
    from cotracker_amd.predictor import choose_replenish
    rel, add, cells = choose_replenish(np.asarray(lost), np.asarray(cover), np.asarray(occupied, dtype=bool), max_lost, max_new)
    assert rel.shape[1:] == (2,) and add.shape[1:] == (2,) and cells.shape == (add.shape[0],)
    return rel.tolist(), add.tolist(), cells.tolist()


def test_choose_replenish_release_threshold():
    occ = [[True] * 6]
    full = [[1] * 4]
    lost = [[0, 2, 3, 4, 8, 3]]
    assert choose(lost, full, occ, 3)[0] == [[0, 2], [0, 3], [0, 4], [0, 5]]  # exactly max_lost is released, one below is not
    assert choose(lost, full, occ, 4)[0] == [[0, 3], [0, 4]]
    assert choose(lost, full, occ, 9) == ([], [], [])
    # an empty slot (-1) is never released, whatever max_lost; nor is a slot the books call free
    assert choose([[-1, -1, 5]], full, [[False, False, True]], 1)[0] == [[0, 2]]
    assert choose([[5, 5, 5]], full, [[False, True, False]], 1)[0] == [[0, 1]]


def test_choose_replenish_cells_and_slots():
    # a 2 x 3 grid: cells 1, 2 and 5 are empty -> row-major order; free slots 1 and 4, and 3 is freed by this call
    cover = [[[2, 0, 0], [1, 1, 0]]]
    occ = [[True, False, True, True, False, True]]
    lost = [[0, -1, 0, 7, -1, 0]]
    rel, add, cells = choose(lost, cover, occ, 4)
    assert rel == [[0, 3]] and add == [[0, 1], [0, 3], [0, 4]] and cells == [1, 2, 5]  # lowest free slots, the freed one included
    assert choose(lost, cover, occ, 8) == ([], [[0, 1], [0, 4]], [1, 2])  # truncated by the free slots
    assert choose(lost, cover, occ, 4, max_new=2) == ([[0, 3]], [[0, 1], [0, 3]], [1, 2])  # by max_new
    assert choose(lost, cover, occ, 4, max_new=0) == ([[0, 3]], [], [])
    assert choose(lost, [[[2, 0, 1], [1, 1, 3]]], occ, 4) == ([[0, 3]], [[0, 1]], [1])  # by the empty cells
    assert choose(lost, [[1] * 6], occ, 4) == ([[0, 3]], [], [])
    flat = choose(lost, [[2, 0, 0, 1, 1, 0]], occ, 4)  # cover given as [G, cells]
    assert flat == (rel, add, cells)


def test_choose_replenish_groups_are_independent():
    cover = [[[0, 1], [1, 0]], [[1, 1], [0, 0]], [[1, 1], [1, 1]]]
    occ = [[True, True, False], [True, False, False], [True, True, True]]
    lost = [[3, 0, -1], [0, -1, -1], [9, 2, 3]]
    rel, add, cells = choose(lost, cover, occ, 3)
    assert rel == [[0, 0], [2, 0], [2, 2]]
    assert add == [[0, 0], [0, 2], [1, 1], [1, 2]] and cells == [0, 3, 2, 3]  # group 2 frees two slots and has no empty cell
    # max_new counts per group
    assert choose(lost, cover, occ, 3, max_new=1)[1:] == ([[0, 0], [1, 1]], [0, 2])
    # the outcome for a group does not depend on the others
    for g in range(3):
        r1, a1, c1 = choose([lost[g]], [cover[g]], [occ[g]], 3)
        assert [[g, n] for _, n in r1] == [r for r in rel if r[0] == g]
        assert [[g, n] for _, n in a1] == [a for a in add if a[0] == g]
        assert c1 == [c for a, c in zip(add, cells) if a[0] == g]


def test_choose_replenish_needs_no_device():
    import inspect
    from cotracker_amd.predictor import choose_replenish
    src = inspect.getsource(choose_replenish)
    assert "torch" not in src.split('"""')[2]  # the body: numpy only
    rel, add, cells = choose_replenish(torch.tensor([[4, -1]]), torch.tensor([[0]]), torch.tensor([[True, False]]), 2)  # host tensors are arrays
    assert rel.tolist() == [[0, 0]] and add.tolist() == [[0, 0]] and cells.tolist() == [0]


# ---- refusals of the model and the predictor ----------------------------------------------------------------------------------------
def test_model_and_predictor_refusals():
    from cotracker_amd.build_cotracker import build_cotracker
    from cotracker_amd.model import CoTrackerThreeOnline
    from cotracker_amd.predictor import CoTrackerOnlinePredictor
    m = CoTrackerThreeOnline(window_len=8, model_resolution=(64, 96))
    first = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no stream is running on the device stream state"):
        m.stream_health(8, (8, 8), 0.6, 3, first, (0.0, 95.0, 0.0, 63.0))
    m.init_video_online_processing()
    with pytest.raises(RuntimeError, match="no stream is running on the device stream state"):
        m.stream_health(8, (8, 8), 0.6, 3, first, (0.0, 95.0, 0.0, 63.0))
    v2 = build_cotracker(None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="stream_health"):
        v2.stream_health(8, (8, 8), 0.6, 3, first, (0.0, 95.0, 0.0, 63.0))
    p = CoTrackerOnlinePredictor(checkpoint=None, window_len=8)
    for call in (lambda: p.track_health(), lambda: p.replenish(2)):  # before any step
        with pytest.raises(RuntimeError, match="no stream is running"):
            call()
    p.spare_points = 2
    p(torch.zeros(1, 1, 3, 32, 48), is_first_step=True, queries=torch.zeros(1, 3, 3))
    for call in (lambda: p.track_health(), lambda: p.replenish(2)):  # after the first step: no window has been tracked
        with pytest.raises(RuntimeError, match="no stream is running"):
            call()
    for bad in (dict(max_lost=0), dict(max_lost=-3), dict(max_lost=5, look=4), dict(max_lost=9), dict(max_lost=2, grid=(64, 65)),
                dict(max_lost=2, grid=(0, 8)), dict(max_lost=2, border=-1.0)):
        with pytest.raises(ValueError):
            p.replenish(**bad)
    for bad in (dict(grid=(4097, 1)), dict(grid=(8, 0)), dict(border=float("nan"))):
        with pytest.raises(ValueError):
            p.track_health(**bad)
    p2 = CoTrackerOnlinePredictor(checkpoint=None, v2=True, window_len=8)
    with pytest.raises(NotImplementedError, match="v2"):
        p2.track_health()
    with pytest.raises(NotImplementedError, match="v2"):
        p2.replenish(2)
