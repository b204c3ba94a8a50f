"""Aggregation inputs and comparisons shared by test_gpu_multiphase.py and
test_gpu_multiphase_dist.py (each keeps its own list of case names)."""
import numpy as np

import _multiphase_ref as ref


def _integral(w):
    return bool(np.all(w == np.round(w)))


def _assert_coarse_equal(got, fine, comm, gmap=None):
    """got = (xadj, tails, w) from the GPU (stitched over the ranks where
    there are several); fine = the aggregated graph."""
    cx, ct, cw, cmap, runs = ref.coarsen(*fine, comm)
    if gmap is not None:
        assert np.array_equal(gmap, cmap)
    assert np.array_equal(got[0], cx)
    assert np.array_equal(got[1], ct)
    if _integral(fine[2]):
        assert np.array_equal(got[2], cw)
        assert got[2].sum() == fine[2].sum()  # total weight conserved
    else:
        bound = (runs - 1) * 2.0 ** -52 * cw
        assert np.all(np.abs(got[2] - cw) <= bound)


def _random_edges(rng, nv, m, lo=0):
    """m random directed edges over vertices [lo, nv): self-loops and
    parallel edges occur, vertices below lo stay isolated."""
    return rng.integers(lo, nv, m), rng.integers(lo, nv, m)


def _coarsen_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("nv"):
        nv = int(name[2:])
        u, v = _random_edges(rng, nv, 4 * nv)
        return nv, u, v, rng.integers(0, nv, nv)
    if name == "no_edges":
        return 5, np.zeros(0, int), np.zeros(0, int), np.array([3, 3, 1, 0, 4])
    if name == "one_community":
        u, v = _random_edges(rng, 100, 600)
        return 100, u, v, np.full(100, 7)
    if name == "identity_parallel":
        u, v = _random_edges(rng, 40, 2000)  # 1600 pairs: many repeats
        return 40, u, v, np.arange(40)
    if name == "sparse_unordered":
        u, v = _random_edges(rng, 300, 2000)
        return 300, u, v, rng.choice([299, 0, 17, 150, 3, 298], 300)
    if name == "isolated_and_loops":
        u, v = _random_edges(rng, 200, 900, lo=50)  # 0..49 isolated
        loops = rng.integers(50, 200, 60)
        return (200, np.r_[u, loops], np.r_[v, loops],
                rng.integers(0, 200, 200))
    if name == "community_of_1000":
        u, v = _random_edges(rng, 1200, 8000)
        return 1200, u, v, np.r_[np.full(1000, 5), np.arange(1000, 1200)]
    if name == "parallel_5000":
        u = np.r_[np.zeros(5000, int), np.ones(5000, int)]
        return 2, u, 1 - u, np.array([1, 0])
    if name == "random_3000":
        u, v = _random_edges(rng, 3000, 40000)
        return 3000, u, v, rng.integers(0, 200, 3000) * 7
    raise KeyError(name)


def _weights(mode, m, seed):
    rng = np.random.default_rng(seed)
    if mode == "unit":
        return np.ones(m)
    if mode == "int":
        return rng.integers(1, 9, m).astype(np.float64)
    return rng.uniform(0.01, 1.0, m)


def _snapshot(h, dist=False):
    """Copy a Hierarchy out into plain Python/numpy data; dist: this rank's
    view, with the parts and global size of every level."""
    L = h.levels
    snap = dict(
        phases=h.phases, levels=L,
        graphs=[None] + [h.graph(k).arrays() for k in range(1, L + 1)],
        maps=[None] + [h.map(k) for k in range(1, L + 1)],
        q=[h.modularity(k) for k in range(L + 1)],
        info=[None] + [h.phase_info(p) for p in range(1, h.phases + 1)],
        communities=h.communities)
    if dist:
        snap.update(
            parts=[None] + [h.graph(k).parts for k in range(1, L + 1)],
            nv=[None] + [h.graph(k).nv for k in range(1, L + 1)])
    return snap


def _snap_equal(a, b):
    def same(x, y):
        if isinstance(x, dict):
            return all(same(x[k], y[k]) for k in x
                       if k not in ("run_ms", "coarsen_ms"))
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, np.ndarray):
            return x.tobytes() == y.tobytes()
        return x == y
    return same(a, b)
