"""CPU yardstick for the tie-heavy / threshold-edge inputs (_tie_graphs.py).

Nothing here touches a GPU. It pins, with the oracle alone, that the inputs
test_gpu_tie_parity.py feeds the engine really are what they are meant to
be: the numpy sweep model reproduces every oracle trace row (so the model
is a faithful restatement of dspl.hpp:174-228), the runs are long enough
and decided by the tie-break often enough (floors), a flipped tie rule
cannot reproduce the oracle's targets (sensitivity), and the oracle's
result does not depend on the partition or on a power-of-two weight scale.
"""
import functools

import numpy as np
import pytest

import _tie_graphs as tg

INPUTS = {
    "composite": tg.composite,
    "composite_relabelled": tg.composite_relabelled,
    "deg256": tg.deg256,
    "dense": tg.dense,
    "lattice_square": tg.lattice_square,
    "lattice_triangular": tg.lattice_triangular,
}
MODES = ("unit", "const2", "ints123")
CASES = [(i, m) for i in INPUTS for m in MODES]

# Floors: (iterations, tie decisions, tie decisions at degree > 256). A tie
# decision is a vertex-iteration whose winning positive gain is shared by
# two or more candidates. The composite/unit floors (8 iterations, 1000
# ties, 50 at hub degree) were fixed when the inputs were designed; const2
# must behave exactly like unit (power-of-two scale). The others are set
# by what each input is FOR, not by the measurement:
#  * a composite-family input is swept for several iterations and must
#    keep hundreds of tie decisions (>= 250), a hub-bearing one at least a
#    handful at hub degree (>= 5) -- ints123 breaks most of the symmetry
#    that unit weights leave, and exits early;
#  * a lattice exits after 2-3 iterations, but with unit weights every
#    vertex ties at iteration 1 (>= nv: 323 / 504);
#  * dense exists for the 24-slot routing; ties are a by-product (>= 20).
# Measured (iterations, ties, hub ties | targets changed by the flipped
# rule, of them at hubs) next to each floor.
FLOORS = {
    ("composite", "unit"): (8, 1000, 50),             # 31, 5099, 192 | 3050, 190
    ("composite", "const2"): (8, 1000, 50),           # 31, 5099, 192 | 3050, 190
    ("composite", "ints123"): (3, 250, 5),            # 4, 845, 20 | 823, 18
    ("composite_relabelled", "unit"): (8, 1000, 50),  # 20, 3819, 124 | 2787, 124
    ("composite_relabelled", "const2"): (8, 1000, 50),  # 20, 3819, 124 | 2787, 124
    ("composite_relabelled", "ints123"): (3, 250, 5),   # 4, 1274, 10 | 955, 9
    ("deg256", "unit"): (8, 1000, 0),                 # 31, 3313, 0 | 2601, 0
    ("deg256", "const2"): (8, 1000, 0),               # 31, 3313, 0 | 2601, 0
    ("deg256", "ints123"): (3, 250, 0),               # 4, 825, 0 | 805, 0
    ("dense", "unit"): (8, 20, 0),                    # 16, 115, 0 | 78, 0
    ("dense", "const2"): (8, 20, 0),                  # 16, 115, 0 | 78, 0
    ("dense", "ints123"): (8, 20, 0),                 # 11, 27, 0 | 22, 0
    ("lattice_square", "unit"): (2, 323, 0),          # 2, 589, 0 | 587, 0
    ("lattice_square", "const2"): (2, 323, 0),        # 2, 589, 0 | 587, 0
    ("lattice_square", "ints123"): (2, 20, 0),        # 4, 288, 0 | 213, 0
    ("lattice_triangular", "unit"): (2, 504, 0),      # 3, 1217, 0 | 1214, 0
    ("lattice_triangular", "const2"): (2, 504, 0),    # 3, 1217, 0 | 1214, 0
    ("lattice_triangular", "ints123"): (2, 20, 0),    # 3, 825, 0 | 676, 0
}


@functools.lru_cache(maxsize=None)
def _base(name):
    return INPUTS[name]()


@functools.lru_cache(maxsize=None)
def _csr(name, mode):
    return tg.WEIGHT_MODES[mode](_base(name))


@functools.lru_cache(maxsize=None)
def _oracle(name, mode, world=1):
    """(mod, iters, targets, mods); read-only for every test."""
    return tg.oracle_run(_csr(name, mode), world)


def _hex(a):
    return [float(x).hex() for x in a]


# ---- the inputs are the ones the GPU cases were designed around ----

def test_input_shapes():
    deg = tg.degrees(_base("composite"))
    assert deg.size == 7561 and deg.max() == 520
    assert int(np.sum(deg > 256)) == 10
    assert {255, 256, 257, 258} <= set(deg.tolist())
    # every hub lies below the cut of the one-rank-skewed case, and the cut
    # leaves ghosts on both sides (it goes through the ring of cliques)
    assert np.flatnonzero(deg > 256).max() < tg.COMPOSITE_RING_CUT
    parts = np.array([0, tg.COMPOSITE_RING_CUT, deg.size])
    for r, (xa, ta, _) in enumerate(tg.split(_base("composite"), parts)):
        remote = (ta < parts[r]) | (ta >= parts[r + 1])
        assert remote.any(), f"rank {r} has no ghosts"
    # the torus is closed: a rank holding exactly it has no ghosts and
    # nobody references it
    xadj, tails, _ = _base("composite")
    src = tg._edges(_base("composite"))[0]
    inside = src < tg.COMPOSITE_TORUS_END
    assert np.all((tails < tg.COMPOSITE_TORUS_END) == inside)
    # relabelling keeps the degree multiset
    assert np.array_equal(np.sort(tg.degrees(_base("composite_relabelled"))),
                          np.sort(deg))
    d = tg.degrees(_base("deg256"))
    assert d.size == 3805 and d.max() == 256  # == 256: not skewed
    xa, ta, _ = _base("dense")
    assert ta.size > 16 * (len(xa) - 1)  # the 24-slot condition
    assert np.all(tg.degrees(_base("lattice_square")) == 4)
    assert np.all(tg.degrees(_base("lattice_triangular")) == 6)


def test_transforms():
    csr = _csr("composite_relabelled", "ints123")
    xadj, tails, w = csr
    src = tg._edges(csr)[0]
    assert np.all(np.diff(tails)[src[1:] == src[:-1]] >= 0)  # rows sorted
    sx, st, sw = tg.shuffle_rows(csr, 3)
    assert np.array_equal(sx, xadj) and not np.array_equal(st, tails)
    unsorted = np.diff(st)[src[1:] == src[:-1]] < 0
    assert unsorted.any()  # rows_sorted == 0 for the engine
    # same multiset of (src, tail, w): weights moved along with their edges
    a = np.lexsort((w, tails, src))
    b = np.lexsort((sw, st, src))
    assert np.array_equal(tails[a], st[b]) and np.array_equal(w[a], sw[b])
    # weights are symmetric: w(u,v) == w(v,u)
    fwd = dict(zip(zip(src.tolist(), tails.tolist()), w.tolist()))
    assert all(fwd[(v, u)] == x for (u, v), x in fwd.items())
    assert set(np.unique(w)) == {1.0, 2.0, 3.0}


# ---- model check, floors, sensitivity ----

@pytest.mark.parametrize("name,mode", CASES)
def test_model_reproduces_oracle(name, mode):
    csr = _csr(name, mode)
    _, iters, tt, _ = _oracle(name, mode)
    rows, _ = tg.replay(csr, tt)
    bad = np.argwhere(rows != tt)
    assert bad.size == 0, (
        f"iteration {bad[0][0] + 1} vertex {bad[0][1]} degree "
        f"{tg.degrees(csr)[bad[0][1]]}: model {rows[tuple(bad[0])]} oracle "
        f"{tt[tuple(bad[0])]}")


@pytest.mark.parametrize("name,mode", CASES)
def test_tie_floors(name, mode):
    csr = _csr(name, mode)
    _, iters, tt, _ = _oracle(name, mode)
    _, tied = tg.replay(csr, tt)
    hub = tg.degrees(csr) > tg.HUB_DEGREE
    ties, hub_ties = int(tied.sum()), int(tied[:, hub].sum())
    print(f"{name}/{mode}: iters {iters} ties {ties} hub ties {hub_ties}")
    f_iters, f_ties, f_hub = FLOORS[(name, mode)]
    assert iters >= f_iters
    assert ties >= f_ties
    assert hub_ties >= f_hub


@pytest.mark.parametrize("name,mode", CASES)
def test_flipped_tie_rule_is_visible(name, mode):
    """Largest-label-wins changes targets on every input, and at a hub on
    the composites: a wrong tie winner cannot pass the parity tests."""
    csr = _csr(name, mode)
    _, _, tt, _ = _oracle(name, mode)
    rows, _ = tg.replay(csr, tt, largest_label_wins=True)
    diff = rows != tt
    hub = tg.degrees(csr) > tg.HUB_DEGREE
    print(f"{name}/{mode}: flipped rule changes {int(diff.sum())} targets, "
          f"{int(diff[:, hub].sum())} at hubs")
    assert diff.any()
    if name.startswith("composite"):
        assert diff[:, hub].any()


# ---- invariances of the oracle itself ----

@pytest.mark.parametrize("name,mode", CASES)
def test_partition_invariance(name, mode):
    mod, iters, tt, tm = _oracle(name, mode)
    for world in (2, 3):
        m2, i2, t2, tm2 = _oracle(name, mode, world)
        assert i2 == iters, f"p={world}"
        assert np.array_equal(t2, tt), f"p={world}"
        assert _hex(tm2) == _hex(tm), f"p={world}"
        assert float(m2).hex() == float(mod).hex(), f"p={world}"


@pytest.mark.parametrize("name", list(INPUTS))
def test_scale_invariance(name):
    """x2.0 is exact, so const2 equals unit bit for bit."""
    mod, iters, tt, tm = _oracle(name, "unit")
    m2, i2, t2, tm2 = _oracle(name, "const2")
    assert i2 == iters and np.array_equal(t2, tt)
    assert _hex(tm2) == _hex(tm) and float(m2).hex() == float(mod).hex()
