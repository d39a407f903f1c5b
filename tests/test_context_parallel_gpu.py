"""Context parallelism on the HIP kernels: two ranks sharing one GPU (gloo, host-staged buffers, ``DLTB_COMM=host``)
with ``--context-parallel 2`` against the world-1 run on the same rows, for every strategy engine (Mistral-shape
``mtiny``, seq 512).  Tolerances: those tests/test_multirank_gpu.py applies to the same strategies."""
import json
import os
import subprocess
import sys

import pytest

from multirank_util import _port, compare, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_multirank_gpu.py
CP_ARGS = ("--seq-len", "512", "--windows", "2")
ALL = "cp_zero2,cp_zero3,cp_ddp,cp_fsdp"
HOST = {"DLTB_COMM": "host"}


@pytest.fixture(scope="module")
def ws1(tmp_path_factory):
    """The world-1 run of every case, computed once."""
    d = tmp_path_factory.mktemp("cp_ws1_gpu")
    return run(d / "ws1.pt", 1, "cuda", extra=CP_ARGS + ("--cases", ALL + ",cp_zero3_window,cp_zero2_doc"), timeout=300)


def test_world2_cp2_equals_world1_gpu(tmp_path, ws1):
    """Every strategy in the default layout (zigzag; contiguous for the windowed case), packed documents included."""
    got = run(tmp_path / "ws2.pt", 2, "cuda", env_extra=HOST, timeout=300,
              extra=CP_ARGS + ("--cases", ALL + ",cp_zero3_window,cp_zero2_doc", "--context-parallel", "2"))
    bad = compare({k: ws1[k] for k in got}, got, **TOL)
    assert not bad, bad


def test_world2_cp2_contiguous_zero3_gpu(tmp_path, ws1):
    got = run(tmp_path / "ws2c.pt", 2, "cuda", env_extra=HOST, timeout=300,
              extra=CP_ARGS + ("--cases", "cp_zero3", "--context-parallel", "2", "--cp-layout", "contiguous"))
    bad = compare({k: ws1[k] for k in got}, got, **TOL)
    assert not bad, bad


def test_world2_cp2_lazy_collectives_gpu(tmp_path, ws1):
    """DLTB_COMM_LAZY=1: an asynchronous collective runs only when its work is waited for, so a layer that read
    K | V before waiting for the gather, or consumed dK | dV before the reduce-scatter, would train another model."""
    got = run(tmp_path / "ws2l.pt", 2, "cuda", env_extra={**HOST, "DLTB_COMM_LAZY": "1"}, timeout=300,
              extra=CP_ARGS + ("--cases", "cp_zero3,cp_zero2", "--context-parallel", "2"))
    bad = compare({k: ws1[k] for k in got}, got, **TOL)
    assert not bad, bad


def test_harness_cp2_end_to_end_gpu(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(HOST)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", "--max-restarts=0", "-m", "dltb.harness",
           "--strategy", "zero3", "--tier", "mtiny", "--seq-len", "512", "--steps", "3", "--warmup-steps", "1",
           "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(tmp_path), "--context-parallel", "2",
           "--tunableop", "off"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    base = tmp_path / "result_zero3_ws2_seq512_tiermtiny"
    with open(f"{base}.json") as f:
        rec = json.load(f)
    with open(f"{base}.extended.json") as f:
        ext = json.load(f)
    assert ext["context_parallel"] == 2 and ext["cp_layout"] == "zigzag"
    assert ext["cp_ranges"] == [[[0, 128], [384, 512]], [[128, 256], [256, 384]]]
    assert ext["tokens_per_micro_step"] == 2 * 512
    assert abs(rec["tokens_per_sec"] * rec["mean_step_time_sec"] - 2 * 512) < 1e-6 * 2 * 512
    assert ext["hip_graphs"] is False
    assert 0.0 < rec["mean_loss"] < 10.0
    assert set(ext["cp_comm_ops_timed"]) == {"all_gather", "reduce_scatter"}
