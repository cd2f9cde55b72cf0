"""tools/bench_batch.py (joint batch mode vs the loop over the videos, measured like a bench.py line): the workload table and the
update_only split without a GPU; on the GPU the keys of a real (smoke-sized) joint-vs-loop line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import bench_batch  # noqa: E402

BATCH_KEYS = ("ms_joint", "ms_loop", "ratio", "spread_joint_ms", "spread_loop_ms", "value_joint", "value_loop",
              "max_abs_diff_joint_vs_loop_px", "update_only_joint", "update_only_loop", "kernels_joint", "hip_kernels_ms",
              "gemm_fraction", "launches_per_call_joint", "batch", "steps")


def test_batch_workloads_are_selectable_and_built_on_baseline_configs():
    assert set(bench_batch.BATCH_WORKLOADS) == {"c4_online_b4", "c2_offline_b8"}
    for name, (base, B, desc) in bench_batch.BATCH_WORKLOADS.items():
        assert base in bench.WORKLOADS and 1 < B <= 16 and name not in bench.WORKLOADS
    assert bench_batch.BATCH_WORKLOADS["c4_online_b4"][:2] == ("c4_online", 4)
    assert bench_batch.BATCH_WORKLOADS["c2_offline_b8"][:2] == ("c2_offline", 8)
    assert bench_batch.WORKLOADS is bench.WORKLOADS  # the base workloads are bench.py's own table, not a copy
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_batch.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "c4_online_b4" in r.stdout and "c2_offline_b8" in r.stdout


def test_update_only_is_the_step_minus_the_encoder():
    u = bench_batch.update_only(1000, 16, 0.050, 10.0)
    assert u["update_ms"] == 40.0 and u["encoder_and_resize_ms"] == 10.0 and abs(u["value"] - 1000 * 16 / 0.040) < 1.0
    assert bench_batch.update_only(1000, 16, 0.050, None) is None and bench_batch.update_only(1000, 16, 0.010, 10.0) is None


@pytest.mark.gpu
def test_keys_of_a_real_joint_vs_loop_line(monkeypatch):
    """A smoke-sized streaming pair through bench_batch.batch_line in a child process (the GPU is opened by the child alone)."""
    code = ("import json, os, sys, torch; sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tools')); import bench_batch as bb\n"
            "bb.WORKLOADS['c4_online'] = (128, 160, 0, 6, False, 8, 'smoke-sized streaming')\n"
            "bb.BATCH_WORKLOADS['c4_online_b4'] = ('c4_online', 3, 'smoke-sized')\n"
            "print(json.dumps(bb.batch_line('c4_online_b4', torch.device('cuda:0'), steps=12, warmup=2)))\n" % (ROOT, ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in BATCH_KEYS + ("graph_nodes",):
        assert k in line, k
    assert line["batch"] == 3 and line["steps"] >= 12 and line["spread_joint_ms"]["calls"] >= 12 and line["spread_loop_ms"]["calls"] >= 12
    assert abs(line["ratio"] - line["ms_joint"] / line["ms_loop"]) < 1e-3
    assert len(line["max_abs_diff_joint_vs_loop_px"]) == 3 and max(line["max_abs_diff_joint_vs_loop_px"]) < 1e-3
    assert line["graph_nodes"]["joint"] > 100 and line["range_fallbacks"] == 0
    assert any(k["name"].startswith("gemm") for k in line["kernels_joint"]) and 0 < line["gemm_fraction"] < 1
