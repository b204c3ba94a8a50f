"""The row queue of the general sweep, on the GPU.

MV_SWEEP_UNIT / MV_SWEEP_GRID are documented as "perf only, results
identical": with a unit of U rows the waves of k4_sweep take their rows
(after a first unit each) from ticket queues instead of a fixed schedule,
and which wave runs which vertex changes from launch to launch. Every
configuration here must reproduce the reference-pinned n=16384 RGG results
(tests/golden/pins.json) exactly as test_gpu_sweep_switches checks them, and
mv_sweep_info must show that every launch drained its queues and no wave
pulled past its first dry ticket: the device ticket words sum to the host's
running total.

The knobs are read at graph load, so they are set in-process and restored
(as test_gpu_degree_windows does for its own).
"""
import os
import threading

import numpy as np
import pytest

import _sweep_child
from test_gpu_degree_windows import _tiny_csr
from test_gpu_sweep_switches import _check

pytestmark = pytest.mark.gpu

KNOBS = ("MV_SWEEP_UNIT", "MV_SWEEP_GRID", "MV_DEG_WINDOW",
         "MV_SWEEP_QUEUE_FROM")
CONFIGS = [(1, True), (1, False), (2, True)]  # (world, unit)
DEFAULT_UNIT_2M = 2  # choose_row_queue's rule at n=2^21 (4 rows per wave)


def _with_knobs(unit, grid, window, fn, queue_from=None):
    """fn() with the knobs set (None: unset); the environment is restored.
    Returns (fn's result, [sweep_info of every engine fn destroyed])."""
    from minivite_amd import Engine
    saved = {k: os.environ.get(k) for k in KNOBS}
    infos, lock, destroy = [], threading.Lock(), Engine.destroy

    def spy(self):
        if getattr(self, "h", None):
            with lock:
                infos.append((self.rank, self.sweep_info()))
        destroy(self)

    try:
        for k, v in zip(KNOBS, (unit, grid, window, queue_from)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        Engine.destroy = spy
        out = fn()
    finally:
        Engine.destroy = destroy
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out, [si for _, si in sorted(infos, key=lambda t: t[0])]


def _check_queue(si, unit, where=""):
    assert si["sched_unit"] == unit, f"{where}{si}"
    assert si["sched_tickets"] == si["sched_tickets_expected"], f"{where}{si}"
    if unit:
        assert si["sched_tickets"] > 0, f"{where}{si}"
    else:
        assert si["sched_tickets"] == 0, f"{where}{si}"


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
    out, infos = _with_knobs(U, grid, window,
                             lambda: _sweep_child.run(world, unit=unit),
                             queue_from=1)
    _check(out, world, unit)
    assert len(infos) == world
    for r, si in enumerate(infos):
        _check_queue(si, U, f"rank {r} ")
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
    from minivite_amd import Graph, Engine
    from oracle.oracle import OracleGraph, louvain, sha
    xadj, tails = _tiny_csr(lnv)
    parts = np.array([0, lnv], dtype=np.int64)
    og = OracleGraph.from_csr(lnv, 1, parts, [(xadj, tails, None)])
    omod, oiters, ott, _ = louvain(og, trace=True)
    og.free()

    def run():
        g = Graph.from_csr(lnv, 0, 1, parts, xadj, tails, None)
        e = Engine(device=0)
        e.load_graph(g)
        e.set_trace(256)
        mod, iters = e.run()
        tt, _ = e.trace(iters)
        e.destroy()
        g.free()
        return mod, iters, tt

    (mod, iters, tt), infos = _with_knobs(2, None, None, run, queue_from=1)
    _check_queue(infos[0], 2)
    rows = (lnv + 63) // 64
    # iteration 1 is the streaming kernel (static); every later one is a
    # k4_sweep launch of one block that takes a ticket per unit
    assert iters >= 2 and infos[0]["general"] == iters - 1
    assert infos[0]["sched_grid"] == 1
    assert infos[0]["sched_tickets"] == (iters - 1) * ((rows + 1) // 2)
    assert iters == oiters
    assert float(mod).hex() == float(omod).hex()
    for k in range(min(iters, 256)):
        assert sha(tt[k]) == sha(ott[k]), f"iter {k + 1}"


@pytest.mark.parametrize("grid", [None, 8])
def test_skewed_graphs_keep_the_static_schedule(grid):
    """Max degree > 256: each thread's spill extent is sized for the
    vertices the static schedule hands it, so a queue asked for by name
    (MV_SWEEP_UNIT=2, from the first k4_sweep launch on) must still be
    refused: sched_unit reads 0, no ticket is taken or expected, and the
    oracle's targets and modularity bits hold (test_gpu_tie_parity._case),
    on the full grid and on a capped one whose threads each take many
    vertices."""
    from test_gpu_tie_parity import _case, _input

    def run():
        return _case(_input("composite_relabelled"),
                     {"skewed": 1, "sched_unit": 0, "sched_tickets": 0,
                      "sched_tickets_expected": 0, "hi": "iters"})

    results, _ = _with_knobs(2, grid, None, run, queue_from=1)
    if grid:
        assert 0 < results[0][4]["sched_grid"] <= grid


def test_repeatability_with_the_queue_on():
    """Which wave runs which rows differs from run to run; the bits of
    every iteration do not."""
    outs = []
    for _ in range(2):
        out, infos = _with_knobs(3, 8, None,
                                 lambda: _sweep_child.run(1, unit=True),
                                 queue_from=1)
        _check_queue(infos[0], 3)
        outs.append(out)
    _check(outs[0], 1, True)
    assert outs[0]["ranks"][0]["iter_mod_hex"] == \
        outs[1]["ranks"][0]["iter_mod_hex"]
    assert outs[0]["iter_target_sha"] == outs[1]["iter_target_sha"]


def test_default_unit():
    """No knob set: a graph with fewer than two units of two rows per wave
    of the full grid keeps the static schedule (n=16384: one row per wave),
    a larger one gets the derived unit (n=2^21: 32768 rows over 8192 waves
    -> U=2) on its steady launches only, and two runs of it agree."""
    from minivite_amd import Graph, Engine
    from oracle.oracle import sha

    def load(nv, runs):
        g = Graph.rgg(nv)
        e = Engine(device=0)
        e.load_graph(g)
        res = []
        for _ in range(runs):
            mod, iters = e.run()
            res.append((float(mod).hex(), iters, sha(e.communities())))
        e.destroy()
        g.free()
        return res

    _, infos = _with_knobs(None, None, None, lambda: load(16384, 0))
    _check_queue(infos[0], 0)
    res, infos = _with_knobs(None, None, None, lambda: load(1 << 21, 2))
    si = infos[0]
    _check_queue(si, DEFAULT_UNIT_2M)
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
    out, infos = _with_knobs(None, 8, None,
                             lambda: _sweep_child.run(1, unit=True))
    _check(out, 1, True)
    si = infos[0]
    _check_queue(si, 4)
    iters = out["ranks"][0]["iters"]
    assert iters > 2
    assert si["sched_tickets"] == (iters - 2) * (256 // 4)
    assert 0 < si["sched_grid"] <= 8
