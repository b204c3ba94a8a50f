"""Every K4 sweep shape on tie-heavy and threshold-edge graphs.

The inputs (_tie_graphs.py, pinned on the CPU by test_tie_graphs_ref.py)
make the tie-break decide thousands of vertex-iterations, at hub degree
too, and sit exactly on the degree-256 routing edge. Every weight is a
small integer, so all sums are exact: each case demands the oracle's
per-iteration targets AND the oracle's modularity bits, and asserts with
Engine.sweep_info() that the kernel shape it exists for is the one that
ran -- a case cannot pass because the dispatch sent its vertices
somewhere else.

When a case fails on targets, the message names the first differing
iteration, vertex and that vertex's degree: degree > 256 is k4_sweep_hi
(unit) / k4_sweep_lh (weighted), anything else k4_sweep_iter1 at
iteration 1 and k4_sweep after it (sweep_info tells which instantiation).
"""
import numpy as np
import pytest

import _tie_graphs as tg
from _gpu_run import in_child
from _sweep_cases import check_parity, check_routing, parity_case as _case

pytestmark = pytest.mark.gpu

_CACHE = {}


def _input(name, mode="unit", shuffled=False):
    """Build each input once per session; read-only afterwards."""
    key = (name, mode, shuffled)
    if key not in _CACHE:
        csr = tg.WEIGHT_MODES[mode](getattr(tg, name)())
        _CACHE[key] = tg.shuffle_rows(csr, 3) if shuffled else csr
    return _CACHE[key]


def _local_hubs(csr, parts):
    deg = tg.degrees(csr)
    return [int(np.sum(deg[lo:hi] > tg.HUB_DEGREE))
            for lo, hi in zip(parts[:-1], parts[1:])]


# ---- hub ties (k4_sweep_hi / k4_sweep_lh), p == 1 ----

# skewed p==1 routing of the general sweep: iteration 1 is the streaming
# kernel, iteration 2 the 12-slot first-iterations variant, the rest 8
SORTED_SKEWED = {"skewed": 1, "rows_sorted": 1, "sell_sorted": 0,
                 "iter1_label_order": 1, "iter1_internal_order": 0,
                 "general": "iters-1", ("slots", 12): 1,
                 ("slots", 8): "iters-2"}


def test_hub_ties_unit():
    """Wave-per-vertex hubs: ties inside wave_reduce_best."""
    _case(_input("composite_relabelled"),
          dict(SORTED_SKEWED, unit_weights=1, nhi=10, nlh=10, hi="iters",
               lh=0))


@pytest.mark.parametrize("mode", ["const2", "ints123"])
def test_hub_ties_weighted(mode):
    """Lane-hash hubs and every UNIT=false instantiation on exact sums."""
    _case(_input("composite_relabelled", mode),
          dict(SORTED_SKEWED, unit_weights=0, nhi=0, nlh=10, lh="iters",
               hi=0))


@pytest.mark.parametrize("mode", ["unit", "const2", "ints123"])
def test_unsorted_rows(mode):
    """rows_sorted == 0 on a skewed graph: no streaming kernel, the general
    sweep runs iteration 1 (12 slots at p == 1) with every neighbour its
    own community."""
    unit = mode == "unit"
    _case(_input("composite_relabelled", mode, shuffled=True),
          {"rows_sorted": 0, "sell_sorted": 0, "skewed": 1,
           "unit_weights": int(unit), "iter1_label_order": 0,
           "iter1_internal_order": 0, "general": "iters", ("slots", 12): 2,
           ("slots", 8): "iters-2", "nlh": 10, "nhi": 10 if unit else 0,
           "hi": "iters" if unit else 0, "lh": 0 if unit else "iters"})


# ---- the degree-256 edge: max degree == 256 is NOT skewed ----

NOT_SKEWED = {"skewed": 0, "nhi": 0, "nlh": 0, "hi": 0, "lh": 0}


@pytest.mark.parametrize("shuffled", [False, True])
def test_boundary_256_unit(shuffled):
    """Unit, not skewed: k_sell_sort_rows puts the rows (sorted or not) in
    internal order and iteration 1 streams them with LBL_ASC=false, which
    finds parallel edges by adjacency."""
    _case(_input("deg256", "unit", shuffled),
          dict(NOT_SKEWED, unit_weights=1, sell_sorted=1,
               rows_sorted=int(not shuffled), iter1_internal_order=1,
               iter1_label_order=0, general="iters-1"))


@pytest.mark.parametrize("mode", ["const2", "ints123"])
def test_boundary_256_weighted(mode):
    _case(_input("deg256", mode),
          dict(NOT_SKEWED, unit_weights=0, sell_sorted=0, rows_sorted=1,
               iter1_label_order=1, iter1_internal_order=0,
               general="iters-1"))


# ---- lattices: nearly every decision is a tie ----

@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("name", ["lattice_square", "lattice_triangular"])
def test_lattices(name, world):
    csr = _input(name)
    _case(csr, {}, parts=tg.even_parts(len(csr[0]) - 1, world))


# ---- p > 1 ----

@pytest.mark.parametrize("mode", ["unit", "const2", "ints123"])
@pytest.mark.parametrize("world", [2, 3])
def test_remote_ties(world, mode):
    """Ties between a local and a remote candidate under label order
    (label_of on the rc_ids side), hubs included."""
    csr = _input("composite_relabelled", mode)
    parts = tg.even_parts(len(csr[0]) - 1, world)
    hubs = _local_hubs(csr, parts)
    assert sum(hubs) == 10 and max(hubs) > 0
    unit = mode == "unit"
    rank_expect = []
    for n in hubs:
        ex = {"skewed": int(n > 0), "nlh": n, "nhi": n if unit else 0}
        if n and unit:
            ex.update(hi=">0", lh=0)
        elif n:
            ex.update(lh=">0", hi=0)
        else:
            ex.update(hi=0, lh=0)
        rank_expect.append(ex)
    _case(csr, {"nghost": ">0", "ssz": ">0", "unit_weights": int(unit)},
          parts=parts, rank_expect=rank_expect)


def test_one_rank_skewed():
    """A locally skewed rank beside a non-skewed one: the overlap decision
    is collective, so neither overlaps."""
    csr = _input("composite")
    parts = [0, tg.COMPOSITE_RING_CUT, len(csr[0]) - 1]
    assert _local_hubs(csr, parts) == [10, 0]
    _case(csr, {"overlap": 0, "nghost": ">0", "ssz": ">0"}, parts=parts,
          rank_expect=[{"skewed": 1, "nhi": 10, "hi": "iters"},
                       {"skewed": 0, "nhi": 0, "nlh": 0, "hi": 0, "lh": 0}])


def test_closed_rank():
    """Rank 0 holds exactly the torus: no ghosts, no exports, the rc
    buffers stay dummies; it still takes part in every collective."""
    csr = _input("composite")
    parts = [0, tg.COMPOSITE_TORUS_END, tg.COMPOSITE_RING_CUT,
             len(csr[0]) - 1]
    results = _case(csr, {}, parts=parts,
                    rank_expect=[{"nghost": 0, "ssz": 0, "skewed": 0},
                                 {"nghost": ">0", "ssz": ">0", "skewed": 1},
                                 {"nghost": ">0", "ssz": ">0", "skewed": 0}])
    overlap = [results[r]["sweep"]["overlap"] for r in range(3)]
    assert overlap[0] == overlap[1] == overlap[2], overlap


# ---- 24 LDS slots (lne > 16 * lnv), weighted and at p > 1 ----

def test_dense_weighted():
    _case(_input("dense", "const2"),
          {**NOT_SKEWED, "unit_weights": 0, "iter1_label_order": 1,
           "general": "iters-1", ("slots", 24): "iters-1"})


def test_dense_unit_p2():
    """Not skewed, exports on both sides: the overlapped halo, where the
    general sweep is launched twice per iteration (exports, interior)."""
    csr = _input("dense")
    results = _case(csr, {**NOT_SKEWED, "unit_weights": 1, "overlap": 1,
                          "nexp": ">0", ("slots", 24): ">0"},
                    parts=tg.even_parts(len(csr[0]) - 1, 2))
    for r, res in results.items():
        info = res["sweep"]
        assert info["general"] == info["general_slots"][24], (r, info)


# ---- k4_sweep_lh<UNIT=true>: reachable only with the band widened ----

def test_lane_hash_unit():
    """MV_LH_THRESH is read once per process: a fresh child runs with the
    lane-hash band widened to degree > 16 (the hubs stay wave-per-vertex)."""
    csr = _input("composite_relabelled")
    results = in_child("tie:composite_relabelled", 1, {"MV_LH_THRESH": "16"})
    info = results[0]["sweep"]
    iters = check_parity(csr, tg.even_parts(len(csr[0]) - 1, 1), results)
    nband = int(np.sum(tg.degrees(csr) > 16))
    assert nband > 10
    check_routing(info, iters, {"nhi": 10, "nlh": nband, "hi": "iters",
                                "lh": "iters", "unit_weights": 1,
                                "skewed": 1})
