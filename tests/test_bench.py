"""bench.py contract: one JSON line with the driver's keys, single process and
a 2-rank gloo run through torch.distributed.run (the multi-GPU launch path,
exercised on CPU)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_single_process(capsys):
    import bench
    assert bench.main(["--full", "--steps", "2", "--warmup", "1", "--classes", "40", "--queries", "12"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert KEYS <= set(rec)
    assert rec["metric"] == "classes indexed/sec" and rec["n_gpus"] == 1 and rec["steps"] == 2
    assert rec["value"] > 0 and rec["higher_is_better"] is True and rec["scaling"] == "weak"
    assert rec["config"]["global_batch"] == 40 and rec["extra"]["classesPerRepo"] == 41
    assert rec["extra"]["graphQueryMs"]["p50"] > 0


def test_bench_plain_run_is_headline_only_and_dumps_its_outputs(capsys, tmp_path):
    """Without --full: the headline alone (no secondary measurement in
    extra), --steps timed steps, and --dump-outputs writes the last step's
    result as float arrays that a second run with the same arguments repeats."""
    import numpy as np
    import bench
    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        assert bench.main(["--steps", "3", "--warmup", "1", "--classes", "40", "--dump-outputs", str(out)]) == 0
        lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
        assert len(lines) == 1
        rec = json.loads(lines[0])
        assert KEYS <= set(rec) and rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert rec["metric"] == "classes indexed/sec" and rec["unit"] == "classes/s"
        # value and ms_per_step describe the same 3 timed steps of 41 classes
        assert rec["value"] == pytest.approx(41 * 1e3 / rec["ms_per_step"], rel=1e-3)
        assert set(rec["extra"]) == {"phaseMsPerStep", "classesPerRepo", "parserThreadsPerRank"}
        files = sorted(p.name for p in out.iterdir())
        assert files == ["analysis.npy", "class_table.npy", "graph_json.npy"]
        dumps.append({f[:-4]: np.load(out / f) for f in files})
    a, b = dumps
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["analysis"][0] == 41 and a["analysis"][2] == 41 and a["class_table"].shape == (41, 5)
    assert a["analysis"][1] == a["class_table"][:, 3].sum() > 0  # endpoints found = endpoint methods in the graph
    graph = json.loads(bytes(a["graph_json"].astype(np.uint8)).decode("utf-8"))
    assert len(graph["nodes"]) == 41 and "co.acme.shop0.order.OrderService" in graph["nodes"]
    for f in a:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.timeout(600)
def test_bench_two_ranks_gloo():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
           "--full", "--steps", "1", "--warmup", "1", "--classes", "30", "--queries", "6"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=540)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 60
    assert rec["config"]["parallelism"].startswith("dp2") and rec["value"] > 0


def test_enrich_pool_extra_deals_one_project_over_every_worker(tmp_path):
    """extra.enrichLocalPool (the production layout: ONE project, ONE pool,
    one worker per GPU), rehearsed with model-free echo workers on the CPU:
    every class enriched, each worker got a share."""
    import bench
    from dmcp.enrich.workers import GpuWorkerPool
    args = bench.parse_args(["--pool-classes", "40"])
    pool = GpuWorkerPool(["cpu"] * 3, {"preset": "echo", "step_s": 0.01, "steps": 1, "max_batch": 64},
                         init=False, start_timeout_s=120)
    try:
        rec = bench._enrich_pool(pool, args, str(tmp_path))
    finally:
        pool.close()
    assert rec["classes"] == 41 and rec["enriched"] == 41 and rec["workers"] == 3
    assert rec["classesPerSec"] > 0 and len(rec["classesPerWorker"]) == 3
    assert all(v > 0 for v in rec["classesPerWorker"].values())
