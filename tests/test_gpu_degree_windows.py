"""The windowed degree order and the row-group sweep schedule, on the GPU.

MV_DEG_WINDOW / MV_DEG_QUANT are documented as "perf only, results
identical": sigma carries the order, and k4_sweep / k4_sweep_iter1 hand each
wave groups of rows instead of a grid stride. Every configuration here must
reproduce the reference-pinned n=16384 RGG results (tests/golden/pins.json)
exactly as _gpu_run.check_vs_pin checks them, while mv_sweep_info reports
the documented effective values and a smaller SELL image.

An explicit MV_DEG_WINDOW is honoured as given (a window longer than lnv is
reported as set and is one short window) with row_group = min(W/64, 8); the
knobs are read at graph load, so they are set in-process and restored.
"""
import numpy as np
import pytest

from _gpu_run import (check_rgg_pin, check_vs_oracle, knobs, run_ranks,
                      run_rgg, traced_run)
from _sweep_cases import tiny_csr

pytestmark = pytest.mark.gpu

CONFIGS = [(1, True), (1, False), (2, True)]  # (world, unit)


def _run_windowed(window, quant, world, unit):
    """The n=16384 RGG with the knobs set (None: unset) -> {rank: record}."""
    with knobs(MV_DEG_WINDOW=window, MV_DEG_QUANT=quant):
        return run_rgg(16384, world, unit)


_plain = {}


def _plain_sell_entries(world, unit):
    """Per-rank SELL entries with the order off; one run per config."""
    if (world, unit) not in _plain:
        records = _run_windowed(0, None, world, unit)
        infos = [records[r]["sweep"] for r in range(world)]
        assert [si["deg_window"] for si in infos] == [0] * world
        assert [si["row_group"] for si in infos] == [1] * world
        _plain[(world, unit)] = [si["sell_entries"] for si in infos]
    return _plain[(world, unit)]


@pytest.mark.parametrize("world,unit", CONFIGS)
@pytest.mark.parametrize("window,quant", [(128, 1), (512, 4), (32768, 1)])
def test_pins_hold_under_degree_windows(window, quant, world, unit):
    plain = _plain_sell_entries(world, unit)
    records = _run_windowed(window, quant, world, unit)
    check_rgg_pin(records, world, unit)
    for r in range(world):
        si = records[r]["sweep"]
        assert si["deg_window"] == window, f"rank {r}"
        assert si["deg_quant"] == quant, f"rank {r}"
        assert si["row_group"] == min(window // 64, 8), f"rank {r}"
        assert 0 < si["sell_entries"] < plain[r], f"rank {r}"


@pytest.mark.parametrize("lnv", [1, 63, 65, 130])
def test_tiny_from_csr_graphs_match_the_oracle(lnv):
    """Partial rows, a row that straddles the only window, isolated
    vertices and a self-loop; compared as test_gpu_parity compares."""
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
        has_hint = g.locality_hint() is not None
        g.free()
        return rec, has_hint

    with knobs(MV_DEG_WINDOW=128, MV_DEG_QUANT=None):
        rec, has_hint = run_ranks(1, body)[0]
    # the order needs a hint, and a one-vertex graph gets none
    assert rec["sweep"]["deg_window"] == (128 if has_hint else 0)
    assert rec["sweep"]["row_group"] == (2 if has_hint else 1)
    check_vs_oracle({0: rec}, oracle, parts)


def test_default_routing_leaves_small_graphs_alone():
    """With no knob set a graph with at most one row per wave keeps the
    plain schedule: every existing small test runs exactly as before."""
    from minivite_amd import Graph

    def load(r, e):
        g = Graph.rgg(16384)
        e.load_graph(g)
        si = e.sweep_info()
        g.free()
        return si

    with knobs(MV_DEG_WINDOW=None, MV_DEG_QUANT=None):
        si = run_ranks(1, load)[0]
    assert si["deg_window"] == 0
    assert si["deg_quant"] == 1
    assert si["row_group"] == 1
    assert si["sell_entries"] > 0
