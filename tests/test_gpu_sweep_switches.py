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

Assertions are those of _gpu_run.check_vs_pin.
"""
import pytest

from _gpu_run import check_rgg_pin, in_child, knobs, run_rgg

pytestmark = pytest.mark.gpu

SPILL_ENV = {"MV_NO_ITER1": "1", "MV_SLOTS": "4", "MV_SLOTS_FIRST": "4"}


@pytest.mark.parametrize("world,unit", [(1, True), (1, False), (2, True)])
def test_general_sweep_at_iteration1_with_spill(world, unit):
    """The switches are static per process: one fresh child per case."""
    records = in_child(f"rgg:16384:{'unit' if unit else 'w'}", world,
                       SPILL_ENV)
    check_rgg_pin(records, world, unit)


@pytest.mark.parametrize("world", [1, 2])
def test_iter1_label_ascending_rows(world):
    """MV_NO_ROWSORT is read at graph load, so it can be set in-process."""
    with knobs(MV_NO_ROWSORT="1"):
        records = run_rgg(16384, world)
    check_rgg_pin(records, world)
