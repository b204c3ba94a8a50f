"""Inputs for the unit-weight slot counts of k4_sweep. Shared by
test_unit_counts_inputs_ref.py (CPU, pins the inputs with the oracle alone)
and test_gpu_unit_counts.py / _engine_child.py.

On a unit graph a k4_sweep slot is {u32 key, u32 count} and the self-loop
and own-community sums are counted outside the ordered edge loop, one pass
per chunk of 8 edges. Every generator returns (xadj, tails, w) with unit
weights; tg.const2 makes the weighted twin. Each input carries the planted
partition and the ring of cliques of _tie_graphs._tail(), which keep the
run alive for many iterations while the gadgets are swept again.
"""
import numpy as np

import _tie_graphs as tg
from _multiphase_ref import csr_from_edges

CH = 8  # edges per chunk of the sweep kernels


def _with_tail(nhead):
    """The tail components behind `nhead` gadget vertices: (csr, offset and
    size of the planted component)."""
    ring, planted = tg._tail()
    tail = tg.union(ring, planted)
    nring = len(ring[0]) - 1
    return tail, nhead + nring, len(planted[0]) - 1


def _assemble(nhead, u, v, loops):
    """Head gadgets [0, nhead) in front of the tail. (u, v): undirected
    pairs, stored in both directions; `loops`: vertices that get ONE
    self-loop entry each (a pair (a, a) in u, v makes two)."""
    tail, _, _ = _with_tail(nhead)
    txadj, ttails, _ = tail
    tsrc = np.repeat(np.arange(len(txadj) - 1, dtype=np.int64),
                     np.diff(txadj)) + nhead
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    loops = np.asarray(loops, dtype=np.int64)
    nv = nhead + len(txadj) - 1
    return csr_from_edges(nv, np.concatenate([u, v, loops, tsrc]),
                          np.concatenate([v, u, loops, ttails + nhead]))


# ---- graph 1: chunk edges ----

CHUNK_DEGREES = (0, 1, 7, 8, 9, 15, 16, 17)
CHUNK_COPIES = 3
CHUNK_HUB_DEGREE = 300


def chunk_layout():
    """{degree: [vertex ids]}, the single- and the double-self-loop vertex
    (both of degree 9), the hub, and the head size."""
    ids, n = {}, 0
    for d in CHUNK_DEGREES:
        ids[d] = list(range(n, n + CHUNK_COPIES))
        n += CHUNK_COPIES
    return ids, n, n + 1, n + 2, n + 3  # ids, loop1, loop2, hub, nhead


def chunk_edges():
    """Vertices of degree 0, 1, 7, 8, 9, 15, 16 and 17 (the chunk edges of
    the 8-wide edge loop) whose neighbours are planted-partition vertices
    reached by 3, 2, 1, 3, 2, 1, ... parallel edges; one vertex with a single
    self-loop entry and one with two; a hub of degree 300, which makes the
    graph skewed, so that the SELL rows keep the input's order. Rows are
    shuffled: with unsorted rows on a skewed graph there is no streaming
    kernel and k4_sweep runs iteration 1 too."""
    ids, loop1, loop2, hub, nhead = chunk_layout()
    _, poff, pn = _with_tail(nhead)
    rng = np.random.default_rng(21)
    u, v = [], []

    def attach(g, d):
        mult, left, k = [], d, 0
        while left:
            mult.append(min((3, 2, 1)[k % 3], left))
            left -= mult[-1]
            k += 1
        nbrs = poff + rng.choice(pn, len(mult), replace=False)
        for nb, mu in zip(nbrs, mult):
            u.extend([g] * mu)
            v.extend([int(nb)] * mu)

    for d in CHUNK_DEGREES:
        for g in ids[d]:
            attach(g, d)
    attach(loop1, 8)  # + 1 self-loop entry = degree 9
    attach(loop2, 7)  # + 2 self-loop entries = degree 9
    u.extend([loop2])
    v.extend([loop2])  # a pair (a, a): two entries
    for nb in poff + rng.choice(pn, CHUNK_HUB_DEGREE, replace=False):
        u.append(hub)
        v.append(int(nb))
    return tg.shuffle_rows(_assemble(nhead, u, v, [loop1]), 5)


# ---- graph 2: slot overflow ----

OVERFLOW_K = tuple(range(5, 14))  # distinct neighbour communities
OVERFLOW_CLIQUE = 6


def overflow_layout():
    """13 cliques of 6 first, then one spoke vertex per k in OVERFLOW_K."""
    ncl = max(OVERFLOW_K)
    spokes = {k: ncl * OVERFLOW_CLIQUE + j for j, k in enumerate(OVERFLOW_K)}
    return ncl, spokes, ncl * OVERFLOW_CLIQUE + len(OVERFLOW_K)


def overflow():
    """Spoke vertex k (k = 5..13) reaches one member of each of k different
    6-cliques, by 1 to 3 parallel edges. Every clique becomes a community of
    its own and stays one, so a spoke keeps seeing its k (later k - 1)
    distinct foreign communities: with 4 LDS slots it increments LDS counts,
    inserts into the spill and increments there, in every iteration. Rows
    sorted, not skewed."""
    ncl, spokes, nhead = overflow_layout()
    iu, iv = np.triu_indices(OVERFLOW_CLIQUE, 1)
    u, v = [], []
    for c in range(ncl):
        u.extend((c * OVERFLOW_CLIQUE + iu).tolist())
        v.extend((c * OVERFLOW_CLIQUE + iv).tolist())
    for k, s in spokes.items():
        for c in range(k):
            member = c * OVERFLOW_CLIQUE + 1 + (k + c) % (OVERFLOW_CLIQUE - 1)
            mu = 1 + (k + 2 * c) % 3
            u.extend([s] * mu)
            v.extend([member] * mu)
    # tie the head to the tail so that it is one component
    _, poff, _ = _with_tail(nhead)
    u.append(0)
    v.append(poff)
    return _assemble(nhead, u, v, [])


# ---- graph 3: count width ----

WIDTH_X = 0          # degree 256: 128 edges into each of two 128-cliques
WIDTH_A0 = 1         # clique A = [1, 129), clique B = [129, 257)
WIDTH_B0 = 129
WIDTH_Y = 257        # 255 parallel edges y - z, one more edge each
WIDTH_Z = 258
WIDTH_HEAD = 259


def count_width():
    """x (label 0) has 128 edges into clique A and 128 into clique B, two
    order-isomorphic 128-cliques: the singleton guard keeps x at home in
    iteration 1, each clique collapses onto its first vertex, and in
    iteration 2 x faces two candidates with count 128 each and equal gains,
    which the label decides. y and z are joined by 255 parallel edges. Max
    degree is 256 (x, y, z): not skewed."""
    iu, iv = np.triu_indices(128, 1)
    u, v = [], []
    for c0 in (WIDTH_A0, WIDTH_B0):
        u.extend((c0 + iu).tolist())
        v.extend((c0 + iv).tolist())
        u.extend([WIDTH_X] * 128)
        v.extend(range(c0, c0 + 128))
    u.extend([WIDTH_Y] * 255)
    v.extend([WIDTH_Z] * 255)
    _, poff, _ = _with_tail(WIDTH_HEAD)
    u.extend([WIDTH_Y, WIDTH_Z])
    v.extend([poff + 3, poff + 77])
    return _assemble(WIDTH_HEAD, u, v, [])


GRAPHS = {"chunk_edges": chunk_edges, "overflow": overflow,
          "count_width": count_width, "dense": tg.dense}
_CACHE = {}


def graph(name, mode="unit"):
    """Build each input once per process; read-only afterwards."""
    if (name, mode) not in _CACHE:
        _CACHE[(name, mode)] = tg.WEIGHT_MODES[mode](GRAPHS[name]())
    return _CACHE[(name, mode)]


def distinct_foreign(csr, curr):
    """Per vertex: the number of distinct neighbour communities other than
    its own under the assignment `curr`."""
    xadj, tails, _ = csr
    nv = len(xadj) - 1
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(xadj))
    curr = np.asarray(curr, dtype=np.int64)
    foreign = curr[tails] != curr[src]
    key = np.unique(src[foreign] * nv + curr[tails][foreign])
    return np.bincount(key // nv, minlength=nv)
