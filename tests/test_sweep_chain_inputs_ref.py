"""CPU yardstick for the row-chain input (_chain_graphs.py). Nothing here
touches a GPU: it pins, with the oracle alone, that the graph
test_gpu_sweep_chain.py feeds the engine is what it is meant to be.
"""
import functools

import numpy as np
import pytest

import _chain_graphs as cg
import _tie_graphs as tg

MODES = ("unit", "ints123")
CASES = [(rem, m) for rem in (0, 1) for m in MODES]


@functools.lru_cache(maxsize=None)
def _run(rem, mode):
    csr = tg.WEIGHT_MODES[mode](cg.chain_graph(rem))
    return csr, tg.oracle_run(csr)


def _distinct_candidates(csr, curr):
    """Per vertex, the number of distinct neighbour communities other than
    its own under the assignment `curr`: the entries the sweep's slot table
    holds for it."""
    xadj, tails, _ = csr
    nv = len(xadj) - 1
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(xadj))
    tcomm = curr[tails]
    key = (src * nv + tcomm)[tcomm != curr[src]]
    return np.bincount(np.unique(key) // nv, minlength=nv)


@pytest.mark.parametrize("rem", [0, 1])
def test_shape(rem):
    xadj, tails, w = cg.chain_graph(rem)
    nv = len(xadj) - 1
    deg = np.diff(xadj)
    assert nv % 64 == rem
    # rows for the one-block queue case: units of three rows, four waves,
    # at least four queued units for each wave
    assert ((nv + 63) // 64 + 2) // 3 - 4 >= 16
    assert {0, 1, 7, 8, 9, 15, 16, 17} <= set(deg.tolist())
    assert deg.max() <= 256  # not skewed: the lane-per-vertex kernels
    z = cg.self_loop_vertex()
    assert np.count_nonzero(tails[xadj[z]:xadj[z + 1]] == z) == 1
    assert np.all(w == 1.0)
    for v in range(nv):  # rows ascending, as the reference CSR
        assert np.all(np.diff(tails[xadj[v]:xadj[v + 1]]) >= 0)
    # the engine's order without a hint: descending degree. One whole slice
    # of 64 positions holds isolated vertices only, so its width is 0.
    by_deg = np.sort(deg)[::-1]
    whole = [c for c in range(nv // 64)
             if by_deg[c * 64:(c + 1) * 64].max() == 0]
    assert whole, "no zero-width slice"
    assert np.count_nonzero(deg == 0) >= cg.ISOLATED_MIN


@pytest.mark.parametrize("rem,mode", CASES)
def test_the_oracle_run_is_what_the_input_is_for(rem, mode):
    csr, (mod, iters, tt, tm) = _run(rem, mode)
    nv = len(csr[0]) - 1
    deg = np.diff(csr[0])
    assert iters >= 4
    ident = np.arange(nv, dtype=np.int64)
    # a mover of degree >= 9 in an iteration >= 3: it passes the second
    # chunk of the edge loop and the move path of a steady launch
    late = [k for k in range(2, iters)
            if np.any((tt[k] != tt[k - 1]) & (deg >= 9))]
    assert late, "no late mover of degree >= 9"
    # under 4 slots the spill holds candidates in iteration 2 ...
    assert np.any(_distinct_candidates(csr, tt[0]) > 4)
    # ... and under the default 8 in some iteration >= 3
    assert any(np.any(_distinct_candidates(csr, tt[k - 1]) > 8)
               for k in range(2, iters))
    # isolated vertices never move
    assert np.all(tt[:iters, deg == 0] == ident[deg == 0])


def test_the_two_sizes_differ_only_in_isolated_vertices():
    a, b = cg.chain_graph(0), cg.chain_graph(1)
    assert len(b[0]) - len(a[0]) == 1
    assert np.array_equal(a[1], b[1])
    for mode in MODES:
        ra, rb = _run(0, mode)[1], _run(1, mode)[1]
        assert ra[1] == rb[1] and float(ra[0]).hex() == float(rb[0]).hex()
