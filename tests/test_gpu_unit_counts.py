"""The unit-weight slot form of k4_sweep: {u32 key, u32 count} slots and the
self-loop / own-community counts taken per chunk of 8 edges.

The inputs (_unit_count_graphs.py, pinned on the CPU by
test_unit_counts_inputs_ref.py) sit on the chunk edges of the edge loop,
overflow the LDS slots into the spill in every iteration, and carry counts
of 128 and 255. Every weight is 1 (or 2 in the weighted twins), so all sums
are exact: each case demands the oracle's targets and its modularity bits
for every iteration, and asserts slot_bytes and general_slots from
Engine.sweep_info(), so that it cannot pass on another kernel.

The knobs that are read once per process go through _gpu_run.in_child().
"""
import pytest

import _tie_graphs as tg
import _unit_count_graphs as ug
from _gpu_run import in_child
from _sweep_cases import check_parity, check_routing, run_parity

pytestmark = pytest.mark.gpu

FOUR_SLOTS = {"MV_SLOTS": "4", "MV_SLOTS_FIRST": "4", "MV_NO_ITER1": "1"}


def _in_process(name, mode, expect):
    csr = ug.graph(name, mode)
    results, iters = run_parity(csr, tg.even_parts(len(csr[0]) - 1, 1))
    check_routing(results[0]["sweep"], iters, expect)
    return iters, results[0]["sweep"]


def _in_child(name, mode, world, env, expect):
    """A fresh process with `env` set; the oracle runs here."""
    csr = ug.graph(name, mode)
    parts = tg.even_parts(len(csr[0]) - 1, world)
    results = in_child(f"unitcount:{name}:{mode}", world, env)
    iters = check_parity(csr, parts, results)
    for r in range(world):
        check_routing(results[r]["sweep"], iters, expect, f"rank {r} ")
    return iters, [results[r]["sweep"] for r in range(world)]


# skewed p == 1 with unsorted rows: k4_sweep runs every iteration, 12 slots
# in the first two and 8 after them; the one hub is wave-per-vertex (unit)
# or lane-hash (weighted)
CHUNK_ROUTING = {"skewed": 1, "rows_sorted": 0, "sell_sorted": 0,
                 "iter1_label_order": 0, "iter1_internal_order": 0,
                 "general": "iters", ("slots", 12): 2,
                 ("slots", 8): "iters-2", "nlh": 1}


def test_chunk_edges_default_slots():
    """Degrees 0, 1, 7, 8, 9, 15, 16, 17, parallel edges inside a chunk and
    across two, one and two self-loop entries; no knob set."""
    _in_process("chunk_edges", "unit",
                dict(CHUNK_ROUTING, unit_weights=1, slot_bytes=8, nhi=1,
                     hi="iters", lh=0))


def test_chunk_edges_weighted_twin():
    _in_process("chunk_edges", "const2",
                dict(CHUNK_ROUTING, unit_weights=0, slot_bytes=12, nhi=0,
                     hi=0, lh="iters"))


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("mode,slot_bytes", [("unit", 8), ("const2", 12)])
def test_slot_overflow(mode, slot_bytes, world):
    """4 LDS slots and the general sweep from iteration 1: the spokes count
    in LDS, insert into the spill and count there. p == 2 is the view-mode
    kernel over loopback."""
    iters, infos = _in_child(
        "overflow", mode, world, FOUR_SLOTS,
        {"skewed": 0, "unit_weights": int(mode == "unit"),
         "slot_bytes": slot_bytes, "iter1_label_order": 0,
         "iter1_internal_order": 0, ("slots", 4): ">0", ("slots", 8): 0,
         ("slots", 12): 0})
    for info in infos:
        assert info["general"] == info["general_slots"][4] >= iters, info
        if world == 2:
            assert info["nghost"] > 0, info


@pytest.mark.parametrize("no_iter1", [False, True])
def test_count_width(no_iter1):
    """A 128 / 128 gain tie at the degree-256 vertex, and 255 parallel edges
    to one neighbour (a slot count of 255 when k4_sweep runs iteration 1).
    The two 128-cliques make the input dense: 24 slots in every launch."""
    expect = {"skewed": 0, "unit_weights": 1, "slot_bytes": 8}
    if no_iter1:
        _in_child("count_width", "unit", 1, {"MV_NO_ITER1": "1"},
                  {**expect, "general": "iters", "iter1_internal_order": 0,
                   "iter1_label_order": 0, ("slots", 24): "iters"})
    else:
        _in_process("count_width", "unit",
                    {**expect, "general": "iters-1",
                     "iter1_internal_order": 1, ("slots", 24): "iters-1"})


def test_dense_takes_24_packed_slots():
    _in_process("dense", "unit",
                {"skewed": 0, "unit_weights": 1, "slot_bytes": 8,
                 "general": "iters-1", ("slots", 24): "iters-1"})
