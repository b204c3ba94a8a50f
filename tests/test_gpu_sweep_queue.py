"""The row queue of the general sweep, on the GPU.

MV_SWEEP_UNIT / MV_SWEEP_GRID are documented as "perf only, results
identical": with a unit of U rows the waves of k4_sweep take their rows
(after a first unit each) from ticket queues instead of a fixed schedule,
and which wave runs which vertex changes from launch to launch. Every
configuration here must reproduce the reference-pinned n=16384 RGG results
(tests/golden/pins.json) exactly as _gpu_run.check_vs_pin checks them, and
mv_sweep_info must show that every launch drained its queues and no wave
pulled past its first dry ticket: the device ticket words sum to the host's
running total.

The knobs are read at graph load, so they are set in-process and restored
(_gpu_run.knobs).
"""
import numpy as np
import pytest

import _tie_graphs as tg
from _gpu_run import (check_rgg_pin, check_vs_oracle, run_ranks, run_rgg,
                      traced_run)
from _sweep_cases import (DEFAULT_UNIT_2M, check_queue, parity_case,
                          queue_knobs, tiny_csr, untraced_runs)

pytestmark = pytest.mark.gpu

CONFIGS = [(1, True), (1, False), (2, True)]  # (world, unit)


# MV_SWEEP_GRID=8: 32 waves take the 256 rows (128 per rank at p=2), many
# units per wave, and U=3 leaves a short last unit. Unset: a row per wave,
# nothing is queued and every ticket finds its queue dry. One configuration
# per (world, unit) also runs over the windowed layout.
# MV_SWEEP_QUEUE_FROM=1 queues every k4_sweep launch (iteration 2 on;
# iteration 1 is the streaming kernel, which never queues), the heavy
# first-iterations launches with their spill traffic included.
@pytest.mark.parametrize("world,unit", CONFIGS)
@pytest.mark.parametrize("grid", [8, None])
@pytest.mark.parametrize("U", [0, 1, 3, 8])
def test_pins_hold_under_the_row_queue(U, grid, world, unit):
    window = 128 if (U, grid) == (3, 8) else None
    with queue_knobs(U, grid, window, queue_from=1):
        records = run_rgg(16384, world, unit)
    check_rgg_pin(records, world, unit)
    for r in range(world):
        si = records[r]["sweep"]
        check_queue(si, U, f"rank {r} ")
        assert si["skewed"] == 0
        if grid:
            assert 0 < si["sched_grid"] <= grid, f"rank {r}"
        elif world == 1:
            assert si["sched_grid"] == 16384 // 256
        else:  # the overlap's second launch covers only the interior
            assert 0 < si["sched_grid"] <= 8192 // 256, f"rank {r}"
        if window:
            assert si["deg_window"] == window and si["row_group"] == 2


@pytest.mark.parametrize("lnv", [1, 63, 65, 130])
def test_tiny_from_csr_graphs_match_the_oracle(lnv):
    """A partial last row, fewer units than waves (most tickets find the
    queue dry) and a range of a single position; compared as
    test_gpu_parity compares."""
    from minivite_amd import Graph
    from oracle.oracle import OracleGraph, louvain
    xadj, tails = tiny_csr(lnv)
    parts = np.array([0, lnv], dtype=np.int64)
    og = OracleGraph.from_csr(lnv, 1, parts, [(xadj, tails, None)])
    oracle = louvain(og, trace=True)
    og.free()

    def body(r, e):
        g = Graph.from_csr(lnv, 0, 1, parts, xadj, tails, None)
        rec, = traced_run(e, g, 256)
        g.free()
        return rec

    with queue_knobs(2, None, queue_from=1):
        records = run_ranks(1, body)
    iters = check_vs_oracle(records, oracle, parts)
    si = records[0]["sweep"]
    check_queue(si, 2)
    rows = (lnv + 63) // 64
    # iteration 1 is the streaming kernel (static); every later one is a
    # k4_sweep launch of one block that takes a ticket per unit
    assert iters >= 2 and si["general"] == iters - 1
    assert si["sched_grid"] == 1
    assert si["sched_tickets"] == (iters - 1) * ((rows + 1) // 2)


@pytest.mark.parametrize("grid", [None, 8])
def test_skewed_graphs_keep_the_static_schedule(grid):
    """Max degree > 256: each thread's spill extent is sized for the
    vertices the static schedule hands it, so a queue asked for by name
    (MV_SWEEP_UNIT=2, from the first k4_sweep launch on) must still be
    refused: sched_unit reads 0, no ticket is taken or expected, and the
    oracle's targets and modularity bits hold (_sweep_cases.parity_case),
    on the full grid and on a capped one whose threads each take many
    vertices."""
    with queue_knobs(2, grid, queue_from=1):
        records = parity_case(
            tg.composite_relabelled(),
            {"skewed": 1, "sched_unit": 0, "sched_tickets": 0,
             "sched_tickets_expected": 0, "hi": "iters"})
    if grid:
        assert 0 < records[0]["sweep"]["sched_grid"] <= grid


def test_repeatability_with_the_queue_on():
    """Which wave runs which rows differs from run to run; the bits of
    every iteration do not."""
    outs = []
    for _ in range(2):
        with queue_knobs(3, 8, queue_from=1):
            records = run_rgg(16384, 1)
        check_queue(records[0]["sweep"], 3)
        outs.append(records)
    check_rgg_pin(outs[0], 1)
    assert outs[0][0]["mods"] == outs[1][0]["mods"]
    assert np.array_equal(outs[0][0]["targets"], outs[1][0]["targets"])


def test_default_unit():
    """No knob set: a graph with fewer than two units of two rows per wave
    of the full grid keeps the static schedule (n=16384: one row per wave),
    a larger one gets the derived unit (n=2^21: 32768 rows over 8192 waves
    -> U=2) on its steady launches only, and two runs of it agree."""
    _, si = untraced_runs(16384, 0)
    check_queue(si, 0)
    res, si = untraced_runs(1 << 21, 2)
    check_queue(si, DEFAULT_UNIT_2M)
    assert res[0] == res[1]
    iters = res[0][1]
    assert iters > 2 and si["general"] == iters - 1
    # iterations 1 and 2 do not queue; each later launch takes a ticket per
    # unit; both runs count (the word is never reset)
    assert si["sched_tickets"] == 2 * (iters - 2) * (32768 // DEFAULT_UNIT_2M)
    assert 0 < si["sched_grid"] <= 2048


def test_default_unit_four_on_a_capped_grid():
    """The shipped bench default, U=4 on the steady launches, at test size:
    with MV_SWEEP_GRID=8 the n=16384 RGG has 8 rows per wave, so the rule
    derives U=4 with no MV_SWEEP_UNIT set. Iterations 1 and 2 stay static;
    every later launch takes one ticket for each of its 64 units; the pins
    hold."""
    with queue_knobs(None, 8):
        records = run_rgg(16384, 1)
    iters = check_rgg_pin(records, 1)
    si = records[0]["sweep"]
    check_queue(si, 4)
    assert iters > 2
    assert si["sched_tickets"] == (iters - 2) * (256 // 4)
    assert 0 < si["sched_grid"] <= 8
