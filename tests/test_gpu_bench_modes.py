"""bench.py's two modes on a small workload: a plain run prints the headline alone (and its --dump-outputs files), --full adds
the fetch check, the loop with the trees left on the device, the single query and the roofline pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--queries", "4", "--n-iter", "3000", "--steps", "2", "--warmup", "1"]


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert d["full"] is False and d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("RRT node-expansions/sec on map_benchmark.pgm", "node-expansions/s", True, "f64")
    for key in ("value_trees_on_device", "roofline", "cpu_baseline"):
        assert key not in d
    assert d["single_query"] is None and d["config"]["fetch_checked"] is None
    for key in ("tamp_queries", "map4_pomdp", "belief_space", "prm_roadmap", "mm_prm"):
        assert key not in d["config"]
    nodes = np.load(tmp_path / "num_nodes.npy")
    assert nodes.dtype == np.float64 and len(nodes) == 4 and np.all(nodes > 1)


def test_full_run_measures_the_extras():
    d = _bench("--full", "--no-pmc", "--no-cpu-baseline", "--no-belief")
    assert d["full"] is True and d["value"] > 0 and d["value_trees_on_device"] > 0
    assert d["config"]["fetch_checked"] is True
    assert d["single_query"]["ms_per_query"] > 0
    assert d["roofline"]["kernel"] in ("k_nn2", "k_conn2") and d["roofline"]["launches"] > 0
