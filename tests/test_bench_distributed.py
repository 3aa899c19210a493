"""bench.py's multi-rank flow, end to end, before any 8-GPU run (VERDICT r02 missing #3).

The driver launches `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` on
one node; this test launches bench.py itself the same way with two ranks on the box's one GPU,
over gloo (RCCL refuses two ranks on one device), and checks what that flow computes:

* rank 0 prints ONE JSON line with n_gpus 2 and the bench contract's keys;
* the ray, sample and C4 counts summed over the ranks equal a one-rank run's (the pass shares
  are disjoint and every sample keeps its key);
* the frame reduced into rank 0 equals the one-rank frame up to float summation order.

The driver's N-GPU runs take the RCCL branch (init_process_group("nccl"), the device-tensor
reduce of the framebuffer, the cuda all-reduces of the totals).  RCCL refuses two ranks on one
device, so test_bench_rccl_one_rank runs that branch with one rank (--force-dist) and checks
that it changes nothing: the same JSON counts and the same frame, bit for bit.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--config", "c3", "--width", "320", "--height", "200", "--spp", "16", "--steps", "2", "--warmup", "1",
        "--full", "--no-cpu-baseline", "--c4-steps", "1"]      # --full: the C4 frames the tests compare


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, env):
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def _check_ranks(out, world, backend):
    """bench.py's per-rank diagnostics (N > 1 / --force-dist): the world RCCL / gloo formed, the
    devices visible, and per rank its frame (render) and framebuffer-reduce times and its samples."""
    r = out["ranks"]
    assert r["world_size"] == world and r["backend"] == backend and r["device_count"] >= 1
    assert [x["rank"] for x in r["per_rank"]] == list(range(world))
    for x in r["per_rank"]:
        fm = x["frame_ms"]
        assert 0 < fm["min"] <= fm["mean"] <= fm["max"]
        assert 0 <= x["reduce_ms"]["mean"] <= x["reduce_ms"]["max"]
        assert x["samples"] > 0 and x["step_ms"] >= fm["mean"]
    assert r["frame_ms_max_over_ranks"] == max(x["frame_ms"]["max"] for x in r["per_rank"])
    assert out["ms_per_step"] >= r["frame_ms_mean_over_ranks"]


@pytest.mark.gpu
def test_bench_two_ranks_match_one(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONUNBUFFERED="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + ARGS + ["--dump-frame", str(tmp_path / "one.npy")], env)
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
                "--dist-backend", "gloo"] + ARGS + ["--dump-frame", str(tmp_path / "two.npy")], env)
    from parity_report import REPORT
    f1, f2 = np.load(tmp_path / "one.npy"), np.load(tmp_path / "two.npy")
    err = float(np.linalg.norm((f1 - f2).astype(np.float64)) / np.linalg.norm(f1.astype(np.float64)))
    REPORT["bench_two_ranks_gloo"] = {"rel_l2_frame": err, "one": {k: one[k] for k in ("value", "ms_per_step")},
                                      "two": {k: two[k] for k in ("value", "ms_per_step")},
                                      "parallelism": two["config"]["parallelism"]}
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "dtype", "config", "roofline"):
        assert k in two, k
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["config"]["parallelism"] == "passes%2+gloo_reduce"
    _check_ranks(two, 2, "gloo")
    assert one["ranks"] is None
    # the per-rank samples add up to the one-rank frame's
    assert sum(r["samples"] for r in two["ranks"]["per_rank"]) == \
        pytest.approx(one["samples_per_s"] * one["ms_per_step"] / 1e3 * two["steps"], rel=1e-3)
    for k in ("closest_hit_rays", "shadow_rays", "traced_rays"):
        assert two[k] == one[k], k
    assert two["samples_per_s"] * two["ms_per_step"] == pytest.approx(one["samples_per_s"] * one["ms_per_step"], rel=1e-3)
    assert (two["c4"]["closest_hit_rays"], two["c4"]["shadow_rays"]) == (one["c4"]["closest_hit_rays"], one["c4"]["shadow_rays"])
    assert err <= 1e-5


@pytest.mark.gpu
def test_bench_rccl_one_rank(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONUNBUFFERED="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    plain = _run([sys.executable, "bench.py", "--gpus", "1"] + ARGS + ["--dump-frame", str(tmp_path / "plain.npy"),
                                                                      "--dump-outputs", str(tmp_path / "out")], env)
    rccl = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                 "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "1",
                 "--dist-backend", "nccl", "--force-dist"] + ARGS + ["--dump-frame", str(tmp_path / "rccl.npy")], env)
    from parity_report import REPORT
    f1, f2 = np.load(tmp_path / "plain.npy"), np.load(tmp_path / "rccl.npy")
    REPORT["bench_rccl_one_rank"] = {"frames_bit_identical": bool(np.array_equal(f1, f2)),
                                     "plain": {k: plain[k] for k in ("value", "ms_per_step")},
                                     "rccl": {k: rccl[k] for k in ("value", "ms_per_step")},
                                     "parallelism": rccl["config"]["parallelism"]}
    assert rccl["config"]["parallelism"] == "passes%1+rccl_reduce"
    assert rccl["n_gpus"] == plain["n_gpus"] == 1
    _check_ranks(rccl, 1, "nccl")
    REPORT["bench_rccl_one_rank"]["ranks"] = rccl["ranks"]
    for k in ("closest_hit_rays", "shadow_rays", "traced_rays", "traversal_stats"):
        assert rccl[k] == plain[k], k
    assert (rccl["c4"]["closest_hit_rays"], rccl["c4"]["shadow_rays"]) == (plain["c4"]["closest_hit_rays"],
                                                                           plain["c4"]["shadow_rays"])
    assert np.array_equal(f1, f2)
    # --dump-outputs: the last timed step's frame and counts (the steps are identical frames)
    out = np.load(tmp_path / "out" / "frame.npy")
    counts = np.load(tmp_path / "out" / "counts.npy")
    assert out.dtype == np.float32 and np.array_equal(out, f1)
    assert counts.dtype == np.float64
    assert (counts[1] * plain["steps"], counts[2] * plain["steps"]) == (plain["closest_hit_rays"], plain["shadow_rays"])
    assert [c * plain["steps"] for c in counts[3:5]] == plain["traced_rays"]
