"""The windowed degree order and the row-group sweep schedule, on the GPU.

MV_DEG_WINDOW / MV_DEG_QUANT are documented as "perf only, results
identical": sigma carries the order, and k4_sweep / k4_sweep_iter1 hand each
wave groups of rows instead of a grid stride. Every configuration here must
reproduce the reference-pinned n=16384 RGG results (tests/golden/pins.json)
exactly as test_gpu_sweep_switches checks them, while mv_sweep_info reports
the documented effective values and a smaller SELL image.

An explicit MV_DEG_WINDOW is honoured as given (a window longer than lnv is
reported as set and is one short window) with row_group = min(W/64, 8); the
knobs are read at graph load, so they are set in-process and restored.
"""
import os
import threading

import numpy as np
import pytest

import _sweep_child
from test_gpu_sweep_switches import _check

pytestmark = pytest.mark.gpu

KNOBS = ("MV_DEG_WINDOW", "MV_DEG_QUANT")
CONFIGS = [(1, True), (1, False), (2, True)]  # (world, unit)


def _with_knobs(window, quant, fn):
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
        for k, v in zip(KNOBS, (window, quant)):
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


_plain = {}


def _plain_sell_entries(world, unit):
    """Per-rank SELL entries with the order off; one run per config."""
    if (world, unit) not in _plain:
        _, infos = _with_knobs(0, None,
                               lambda: _sweep_child.run(world, unit=unit))
        assert [si["deg_window"] for si in infos] == [0] * world
        assert [si["row_group"] for si in infos] == [1] * world
        _plain[(world, unit)] = [si["sell_entries"] for si in infos]
    return _plain[(world, unit)]


@pytest.mark.parametrize("world,unit", CONFIGS)
@pytest.mark.parametrize("window,quant", [(128, 1), (512, 4), (32768, 1)])
def test_pins_hold_under_degree_windows(window, quant, world, unit):
    plain = _plain_sell_entries(world, unit)
    out, infos = _with_knobs(window, quant,
                             lambda: _sweep_child.run(world, unit=unit))
    _check(out, world, unit)
    assert len(infos) == world
    for r, si in enumerate(infos):
        assert si["deg_window"] == window, f"rank {r}"
        assert si["deg_quant"] == quant, f"rank {r}"
        assert si["row_group"] == min(window // 64, 8), f"rank {r}"
        assert 0 < si["sell_entries"] < plain[r], f"rank {r}"


def _tiny_csr(lnv):
    """A chordal ring over the vertices that are not isolated (every 7th
    is), with a self-loop on vertex 0. Rows ascending, symmetric."""
    live = [v for v in range(lnv) if v % 7 != 3]
    pairs = {(0, 0)}
    for k, v in enumerate(live):
        for step in (1, 3):
            u = live[(k + step) % len(live)]
            if u != v:
                pairs.add((v, u))
                pairs.add((u, v))
    pairs = sorted(pairs)
    xadj = np.zeros(lnv + 1, dtype=np.int64)
    for v, _ in pairs:
        xadj[v + 1] += 1
    return np.cumsum(xadj), np.array([u for _, u in pairs], dtype=np.int64)


@pytest.mark.parametrize("lnv", [1, 63, 65, 130])
def test_tiny_from_csr_graphs_match_the_oracle(lnv):
    """Partial rows, a row that straddles the only window, isolated
    vertices and a self-loop; compared as test_gpu_parity compares."""
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
        has_hint = g.locality_hint() is not None
        e.destroy()
        g.free()
        return mod, iters, tt, has_hint

    (mod, iters, tt, has_hint), infos = _with_knobs(128, None, run)
    # the order needs a hint, and a one-vertex graph gets none
    assert infos[0]["deg_window"] == (128 if has_hint else 0)
    assert infos[0]["row_group"] == (2 if has_hint else 1)
    assert iters == oiters
    assert float(mod).hex() == float(omod).hex()
    for k in range(min(iters, 256)):
        assert sha(tt[k]) == sha(ott[k]), f"iter {k + 1}"


def test_default_routing_leaves_small_graphs_alone():
    """With no knob set a graph with at most one row per wave keeps the
    plain schedule: every existing small test runs exactly as before."""
    from minivite_amd import Graph, Engine

    def load():
        g = Graph.rgg(16384)
        e = Engine(device=0)
        e.load_graph(g)
        e.destroy()
        g.free()

    _, infos = _with_knobs(None, None, load)
    assert infos[0]["deg_window"] == 0
    assert infos[0]["deg_quant"] == 1
    assert infos[0]["row_group"] == 1
    assert infos[0]["sell_entries"] > 0
