"""K4 sweep instantiations that the default configuration never launches.

The sweep tunables are documented as "perf only, results identical", so
every configuration here must reproduce the reference-pinned n=16384 RGG
results in tests/golden/pins.json:

* MV_NO_ITER1 + 4 LDS slots: the general sweep runs iteration 1, where every
  neighbour is its own community — at average degree ~10 most lanes overflow
  4 slots into the global spill region (k4_sweep<MR, 4, UNIT>, both modes,
  both weight kinds).
* MV_NO_ROWSORT: the iteration-1 streaming kernel over label-ascending rows
  (k4_sweep_iter1<MR, UNIT=true, LBL_ASC=true>) on a non-skewed graph.

Assertions are those of test_gpu_parity.test_single_gpu_parity_* and
test_gpu_loopback._check_vs_pin.
"""
import json
import os
import subprocess
import sys

import pytest

import _sweep_child

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pins.json")
SPILL_ENV = {"MV_NO_ITER1": "1", "MV_SLOTS": "4", "MV_SLOTS_FIRST": "4"}


def _pin_key(world, unit):
    return f"rgg_n16384_p{world}_{'unit' if unit else 'w'}"


def _check(out, world, unit):
    pin = json.load(open(GOLDEN))[_pin_key(world, unit)]
    iters = out["ranks"][0]["iters"]
    assert iters == pin["iters"]
    assert len(out["ranks"]) == world
    for r, rk in enumerate(out["ranks"]):  # every rank agrees
        assert rk["iters"] == iters
        if unit:
            assert rk["final_mod_hex"] == pin["final_mod_hex"], f"rank {r}"
            assert rk["iter_mod_hex"] == pin["iter_mod_hex"], f"rank {r}"
        else:
            assert abs(float.fromhex(rk["final_mod_hex"])
                       - float.fromhex(pin["final_mod_hex"])) < 1e-9
    assert out["iter_target_sha"] == pin["iter_target_sha"]
    if world == 1:
        assert out["sweep_launches"] == iters


@pytest.mark.parametrize("world,unit", [(1, True), (1, False), (2, True)])
def test_general_sweep_at_iteration1_with_spill(world, unit):
    """The switches are static per process: one fresh child per case."""
    env = dict(os.environ, **SPILL_ENV)
    child = subprocess.run(
        [sys.executable, _sweep_child.__file__, str(world),
         "unit" if unit else "w"],
        env=env, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    _check(json.loads(child.stdout.strip().splitlines()[-1]), world, unit)


@pytest.mark.parametrize("world", [1, 2])
def test_iter1_label_ascending_rows(world):
    """MV_NO_ROWSORT is read at graph load, so it can be set in-process."""
    os.environ["MV_NO_ROWSORT"] = "1"
    try:
        out = _sweep_child.run(world, unit=True)
    finally:
        del os.environ["MV_NO_ROWSORT"]
    _check(out, world, unit=True)
