"""bench.py's plain run and --dump-outputs on the GPU: a small C2 shard, twice.

A plain run measures the headline only (no parity, roofline or other leg: those are --full's) and
with --dump-outputs DIR writes the last timed slot's outputs; the inputs come from fixed seeds, so
two runs with the same arguments write the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, N = 500, 4


def _run(out_dir, steps):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2", "--validators", str(V),
           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=200)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    (line,) = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    return line


def test_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    a, b = _run(tmp_path / "a", 2), _run(tmp_path / "b", 4)  # the last slot lands on another in-flight set
    for line, steps in ((a, 2), (b, 4)):
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["full"] is False and line["parity"] is None and line["roofline"] is None
        assert line["kernels"] is None and line["cpu_baseline"] is None
        assert not {"with_key_tables", "verify_aggregate", "concurrent_callers", "host_buffer_items_per_s"} & set(line)
    shapes = {"verify_status": (V * N, 1), "aggregates": (V, 96), "aggregate_status": (V, 1),
              "aggregate_verify_status": (V, 1), "signing_roots": (64, 32)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in shapes)
    for k, shape in shapes.items():
        x, y = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert x.dtype == np.float32 and x.shape == shape and np.array_equal(x, y), k
    for k in ("verify_status", "aggregate_status", "aggregate_verify_status"):
        assert not np.load(tmp_path / "a" / f"{k}.npy").any(), k  # every item OK
    agg = np.load(tmp_path / "a" / "aggregates.npy")
    assert agg.any() and len({bytes(r.astype(np.uint8)) for r in agg}) == V  # V distinct signatures
