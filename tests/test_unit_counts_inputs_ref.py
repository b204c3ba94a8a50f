"""CPU yardstick for the unit-count inputs (_unit_count_graphs.py).

Nothing here touches a GPU. It pins, with the oracle and numpy alone, that
the inputs test_gpu_unit_counts.py feeds the engine do what they exist for:
the chunk-edge degrees, parallel edges inside one chunk of 8 and across
two, both self-loop forms, spokes that overflow 4 slots in iteration after
iteration, a degree-256 vertex whose 128/128 split is decided by the label,
and runs long enough to reach the steady slot count.
"""
import functools

import numpy as np
import pytest

import _tie_graphs as tg
import _unit_count_graphs as ug

MIN_ITERS = 3


@functools.lru_cache(maxsize=None)
def _oracle(name, mode="unit"):
    """(mod, iters, targets, mods); read-only for every test."""
    return tg.oracle_run(ug.graph(name, mode))


def _curr(tt, k, nv):
    """The assignment iteration k + 1 starts from."""
    return np.arange(nv, dtype=np.int64) if k == 0 else tt[k - 1]


def _row(csr, v):
    return csr[1][csr[0][v]:csr[0][v + 1]]


@pytest.mark.parametrize("name,mode", [
    ("chunk_edges", "unit"), ("chunk_edges", "const2"),
    ("overflow", "unit"), ("overflow", "const2"),
    ("count_width", "unit"), ("dense", "unit")])
def test_runs_are_long_enough(name, mode):
    _, iters, _, _ = _oracle(name, mode)
    print(f"{name}/{mode}: {iters} iterations")
    assert iters >= MIN_ITERS


def test_chunk_edges_shape():
    csr = ug.graph("chunk_edges")
    ids, loop1, loop2, hub, nhead = ug.chunk_layout()
    deg = tg.degrees(csr)
    assert deg.size <= 4000
    for d, vs in ids.items():
        assert [int(deg[v]) for v in vs] == [d] * len(vs)
    assert deg[hub] == ug.CHUNK_HUB_DEGREE
    assert int(np.sum(deg > tg.HUB_DEGREE)) == 1  # skewed, by the hub alone
    # self-loop entries: one, and two
    assert int(np.sum(_row(csr, loop1) == loop1)) == 1 and deg[loop1] == 9
    assert int(np.sum(_row(csr, loop2) == loop2)) == 2 and deg[loop2] == 9
    # rows are unsorted
    src = tg._edges(csr)[0]
    assert (np.diff(csr[1])[src[1:] == src[:-1]] < 0).any()
    # a neighbour twice or more inside one chunk, and one in two chunks
    inside = across = 0
    for d in (9, 15, 16, 17):
        for v in ids[d]:
            row = _row(csr, v)
            first, second = row[:ug.CH], row[ug.CH:2 * ug.CH]
            inside += int(np.unique(first).size < first.size)
            across += int(np.intersect1d(first, second).size > 0)
    print(f"rows with a repeat inside chunk 0: {inside}, across: {across}")
    assert inside >= 1 and across >= 1


def test_chunk_edges_counts_matter():
    """A gadget's candidate sums exceed 1 in every iteration: they are the
    parallel-edge counts."""
    csr = ug.graph("chunk_edges")
    ids, _, _, _, _ = ug.chunk_layout()
    for v in ids[17]:
        _, cnt = np.unique(_row(csr, v), return_counts=True)
        assert cnt.max() == 3 and cnt.min() == 1


def test_overflow_spokes_overflow():
    """More than 4 distinct foreign communities at the spokes in at least
    two iterations after the first (the first has them by construction:
    every neighbour is its own community)."""
    csr = ug.graph("overflow")
    nv = len(csr[0]) - 1
    assert nv <= 4000 and tg.degrees(csr).max() <= tg.HUB_DEGREE
    _, spokes, _ = ug.overflow_layout()
    for k, s in spokes.items():
        row, cnt = np.unique(_row(csr, s), return_counts=True)
        assert row.size == k and 1 <= cnt.min() and cnt.max() <= 3
    _, iters, tt, _ = _oracle("overflow")
    over = []
    for k in range(iters):
        nd = ug.distinct_foreign(csr, _curr(tt, k, nv))
        over.append(int(np.sum(nd[list(spokes.values())] > 4)))
    print(f"spokes above 4 distinct foreign communities, per iteration: "
          f"{over}")
    assert over[0] == len(spokes)
    assert sum(1 for n in over[1:] if n > 0) >= 2
    # and some spoke has parallel edges both to a community that sits in an
    # LDS slot and to one that spills: more than 4 neighbours with count > 1
    s13 = spokes[13]
    _, cnt = np.unique(_row(csr, s13), return_counts=True)
    assert int(np.sum(cnt > 1)) > 4


def test_count_width_ties():
    """The degree-256 vertex faces a 128 / 128 split with equal gains in an
    iteration that k4_sweep runs (any but the first)."""
    csr = ug.graph("count_width")
    deg = tg.degrees(csr)
    assert deg.size <= 4000 and deg.max() == 256  # == 256: not skewed
    assert deg[ug.WIDTH_X] == 256
    assert csr[1].size > 16 * deg.size  # the cliques make it a 24-slot input
    row = _row(csr, ug.WIDTH_X)
    assert int(np.sum((row >= ug.WIDTH_A0) & (row < ug.WIDTH_B0))) == 128
    assert int(np.sum(row >= ug.WIDTH_B0)) == 128
    assert int(np.sum(_row(csr, ug.WIDTH_Y) == ug.WIDTH_Z)) == 255
    assert int(np.sum(_row(csr, ug.WIDTH_Z) == ug.WIDTH_Y)) == 255
    _, iters, tt, _ = _oracle("count_width")
    _, tied = tg.replay(csr, tt)
    nv = deg.size
    hits = []
    for k in range(1, iters):
        curr = _curr(tt, k, nv)
        a, b = curr[ug.WIDTH_A0], curr[ug.WIDTH_B0]
        split = (np.all(curr[ug.WIDTH_A0:ug.WIDTH_B0] == a)
                 and np.all(curr[ug.WIDTH_B0:ug.WIDTH_Y] == b) and a != b
                 and curr[ug.WIDTH_X] not in (a, b))
        if split and tied[k, ug.WIDTH_X]:
            hits.append(k + 1)
            assert tt[k, ug.WIDTH_X] == min(a, b)  # the label decided
    print(f"x ties 128/128 in iterations {hits}")
    assert hits


def test_dense_takes_24_slots():
    xa, ta, _ = ug.graph("dense")
    assert ta.size > 16 * (len(xa) - 1)
