"""bench.py's command line: a plain run prints the result line without the
--full extras, --steps sets the number of timed steps, and --dump-outputs
writes the last timed step's outputs — checked against the reference-pinned
fixture (tests/golden/pins.json) on the smallest pinned graph."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pins.json")


def _bench(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                           *argv], capture_output=True, text=True,
                          timeout=300)


def test_bench_rejects_zero_steps():
    out = _bench("--steps", "0")
    assert out.returncode != 0
    assert "--steps" in out.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_pinned_outputs(tmp_path):
    from oracle.oracle import sha
    pin = json.load(open(GOLDEN))["rgg_n16384_p1_unit"]
    d = tmp_path / "dump"
    out = _bench("--gpus", "1", "--steps", "3", "--warmup", "1",
                 "--nv", "16384", "--dump-outputs", str(d))
    assert out.returncode == 0, out.stderr[-800:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["metric"] == "Louvain-iter edges/s"
    assert res["unit"] == "edges*iters/s"
    assert res["higher_is_better"] is True
    assert res["dtype"] == "f64"
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    # value is edges x iterations per second of one timed step
    want = (res["config"]["directed_edges"] * res["config"]["iterations"]
            / (res["ms_per_step"] * 1e-3))
    assert abs(res["value"] - want) <= 1e-9 * want
    assert res["cpu_baseline"] is None  # --full only

    got = {n: np.load(d / (n + ".npy")) for n in
           ("modularity", "iterations", "iter_modularity", "communities")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["iterations"].tolist() == [pin["iters"]]
    assert [float(m).hex() for m in got["modularity"]] == [pin["final_mod_hex"]]
    assert [float(m).hex() for m in got["iter_modularity"]] \
        == pin["iter_mod_hex"]
    assert sha(got["communities"].astype(np.int64)) \
        == pin["iter_target_sha"][-1]
