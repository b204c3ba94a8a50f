"""Tie-heavy and threshold-edge graphs for the sweep kernels, plus a numpy
restatement of one sweep decision. Shared by test_tie_graphs_ref.py (CPU,
pins the inputs with the oracle alone) and test_gpu_tie_parity.py.

Every generator returns (xadj, tails, w) with rows sorted by tail and
unit weights; the weight modes are applied on top (const2, ints123). All
weights used here are small integers, so every sum the engine, the oracle
and the model form is exact in double precision.

The Louvain loop exits on GLOBAL modularity, and a lattice or a biclique
alone oscillates and exits at iteration 2. The composite inputs are
disjoint unions with a planted-partition component that keeps the run
alive while the tie-heavy components are swept again every iteration.
"""
import numpy as np

from _multiphase_ref import csr_from_edges, planted, ring_of_cliques, symmetric

HUB_DEGREE = 256  # the engine's skewed / hub-band threshold (degree > 256)


# ---- generators ----

def torus(R, C):
    """4-regular wrap-around lattice: every iteration-1 gain ties."""
    r, c = np.divmod(np.arange(R * C), C)
    right = r * C + (c + 1) % C
    down = ((r + 1) % R) * C + c
    me = np.arange(R * C)
    return symmetric(R * C, np.concatenate([me, me]),
                     np.concatenate([right, down]))


def tri_torus(R, C):
    """6-regular triangular wrap-around lattice (torus + one diagonal)."""
    r, c = np.divmod(np.arange(R * C), C)
    right = r * C + (c + 1) % C
    down = ((r + 1) % R) * C + c
    diag = ((r + 1) % R) * C + (c + 1) % C
    me = np.arange(R * C)
    return symmetric(R * C, np.concatenate([me, me, me]),
                     np.concatenate([right, down, diag]))


def bicliques(sizes, hubs):
    """One block per L in `sizes`: `hubs` hub vertices, each joined to the
    same L leaves (hub degree == L exactly). Even blocks put the hubs below
    their leaves in label order, odd blocks above. The blocks are joined by
    a ring through leaf 0 of each (a single edge for two blocks)."""
    u, v, first_leaf, base = [], [], [], 0
    for b, L in enumerate(sizes):
        if b % 2 == 0:
            hub0, leaf0 = base, base + hubs
        else:
            leaf0, hub0 = base, base + L
        hh = np.repeat(np.arange(hub0, hub0 + hubs), L)
        ll = np.tile(np.arange(leaf0, leaf0 + L), hubs)
        u.append(hh)
        v.append(ll)
        first_leaf.append(leaf0)
        base += hubs + L
    n = len(sizes)
    ring = [(k, (k + 1) % n) for k in range(n)] if n > 2 else \
        [(0, 1)] if n == 2 else []
    u.append(np.array([first_leaf[a] for a, _ in ring], dtype=np.int64))
    v.append(np.array([first_leaf[b] for _, b in ring], dtype=np.int64))
    return symmetric(base, np.concatenate(u), np.concatenate(v))


def hub_of_cliques(Ms, k, hubs):
    """One block per M in `Ms`: M k-cliques, then `hubs` hub vertices each
    joined to vertex 0 of every clique (hub degree == M exactly). Once the
    cliques have merged, a hub faces M identical candidates in every later
    iteration."""
    iu, iv = np.triu_indices(k, 1)
    u, v, base = [], [], 0
    for M in Ms:
        cb = base + np.arange(M)[:, None] * k
        u.append((cb + iu[None, :]).ravel())
        v.append((cb + iv[None, :]).ravel())
        hub0 = base + M * k
        u.append(np.repeat(np.arange(hub0, hub0 + hubs), M))
        v.append(np.tile(base + np.arange(M) * k, hubs))
        base = hub0 + hubs
    return symmetric(base, np.concatenate(u), np.concatenate(v))


def union(*csrs):
    """Disjoint union, ids offset in argument order."""
    xs, ts, ws, off, eoff = [np.zeros(1, np.int64)], [], [], 0, 0
    for xadj, tails, w in csrs:
        xs.append(xadj[1:] + eoff)
        ts.append(tails + off)
        ws.append(w)
        off += len(xadj) - 1
        eoff += len(tails)
    return np.concatenate(xs), np.concatenate(ts), np.concatenate(ws)


def _edges(csr):
    xadj, tails, w = csr
    src = np.repeat(np.arange(len(xadj) - 1, dtype=np.int64), np.diff(xadj))
    return src, tails, w


def relabel(csr, seed):
    """Random vertex permutation; rows re-sorted by (new) tail."""
    nv = len(csr[0]) - 1
    perm = np.random.default_rng(seed).permutation(nv)
    src, tails, w = _edges(csr)
    return csr_from_edges(nv, perm[src], perm[tails], w)


def shuffle_rows(csr, seed):
    """Random edge order inside every row; weights move along."""
    xadj, tails, w = csr
    src = _edges(csr)[0]
    key = np.random.default_rng(seed).random(tails.size)
    order = np.lexsort((key, src))
    return xadj.copy(), tails[order].copy(), w[order].copy()


def split(csr, parts):
    """Per-rank (xadj, tails, w) of the 1-D partition `parts`."""
    xadj, tails, w = csr
    out = []
    for lo, hi in zip(parts[:-1], parts[1:]):
        out.append(((xadj[lo:hi + 1] - xadj[lo]).copy(),
                    tails[xadj[lo]:xadj[hi]].copy(),
                    None if w is None else w[xadj[lo]:xadj[hi]].copy()))
    return out


def even_parts(nv, world):
    return np.array([(nv * r) // world for r in range(world + 1)],
                    dtype=np.int64)


# ---- weight modes (both directions of a pair agree) ----

def const2(csr):
    xadj, tails, w = csr
    return xadj, tails, np.full(tails.size, 2.0)


def ints123(csr):
    """Integers 1..3 from (min(u,v), max(u,v))."""
    src, tails, _ = _edges(csr)
    lo, hi = np.minimum(src, tails), np.maximum(src, tails)
    return csr[0], tails, (1 + (lo + hi) % 3).astype(np.float64)


WEIGHT_MODES = {"unit": lambda csr: csr, "const2": const2, "ints123": ints123}


# ---- the inputs ----

def _tail():
    return (ring_of_cliques(40, 5),
            planted(seed=12, nblocks=40, bsize=50, npairs=8000))


def composite():
    """nv 7561; hubs of degree 255..258, 300 and 520; 10 vertices above
    degree 256. Component offsets: torus 0, hub_of_cliques 320, bicliques
    4327, ring_of_cliques 5361, planted 5561."""
    return union(torus(16, 20),
                 hub_of_cliques([256, 257, 300, 520], k=3, hubs=2),
                 bicliques([255, 256, 257, 258], hubs=2), *_tail())


COMPOSITE_TORUS_END = 320    # rank 0 of the closed-rank case
COMPOSITE_RING_CUT = 5361 + 100  # inside the ring of cliques, past every hub
RELABEL_SEED = 6


def composite_relabelled():
    return relabel(composite(), RELABEL_SEED)


def deg256():
    """The composite with only the degree <= 256 hub blocks: max degree is
    exactly 256, so the engine must NOT treat it as skewed. nv 3805."""
    return union(torus(16, 20), hub_of_cliques([256], k=3, hubs=2),
                 bicliques([255, 256], hubs=2), *_tail())


def dense():
    """planted() defaults: more than 16 edges per vertex (24 LDS slots)."""
    return planted()


def lattice_square():
    return torus(17, 19)


def lattice_triangular():
    return tri_torus(21, 24)


# ---- one sweep decision per vertex, in numpy ----

def degrees(csr):
    return np.diff(csr[0])


def sweep_model(csr, curr, largest_label_wins=False):
    """targetComm of every vertex for one iteration that starts from the
    assignment `curr` (the previous trace row; the identity at iteration
    1), following distGetMaxIndex (dspl.hpp:174-228):

      gain(y) = 2*(e_iy - e_ix) - 2*vdeg*(a_y - a_x)*constant,  y != cc
      the largest gain > 0 wins; equal gains go to the smallest label;
      a singleton moving into a singleton with a larger label stays.

    Community degree/size are recomputed from `curr`, which equals the
    incrementally maintained cinfo when every weight is an integer.
    Returns (target, tied): tied[v] is True where the winning positive
    gain was shared by two or more candidates. `largest_label_wins` flips
    the tie rule (for the sensitivity check only)."""
    xadj, tails, w = csr
    nv = len(xadj) - 1
    src, _, _ = _edges(csr)
    curr = np.asarray(curr, dtype=np.int64)
    vdeg = np.bincount(src, weights=w, minlength=nv)
    constant = 1.0 / float(np.sum(w))
    adeg = np.bincount(curr, weights=vdeg, minlength=nv)
    size = np.bincount(curr, minlength=nv)
    selfloop = np.bincount(src[src == tails], weights=w[src == tails],
                           minlength=nv)
    tcomm = curr[tails]
    own = tcomm == curr[src]
    c0 = np.bincount(src[own], weights=w[own], minlength=nv)
    eix = c0 - selfloop
    ax = adeg[curr] - vdeg
    # one candidate per distinct (vertex, neighbour community != cc)
    key = src[~own] * nv + tcomm[~own]
    ukey, inv = np.unique(key, return_inverse=True)
    eiy = np.bincount(inv, weights=w[~own], minlength=ukey.size)
    cv, cy = ukey // nv, ukey % nv
    gain = 2.0 * (eiy - eix[cv]) - 2.0 * vdeg[cv] * (adeg[cy] - ax[cv]) \
        * constant
    best = np.zeros(nv)
    np.maximum.at(best, cv, gain)           # max(0, gains): 0 never wins
    winners = (gain == best[cv]) & (gain > 0.0)
    nwin = np.bincount(cv[winners], minlength=nv)
    target = curr.copy()
    if largest_label_wins:
        pick = np.full(nv, -1, dtype=np.int64)
        np.maximum.at(pick, cv[winners], cy[winners])
    else:
        pick = np.full(nv, nv, dtype=np.int64)
        np.minimum.at(pick, cv[winners], cy[winners])
    moved = nwin > 0
    target[moved] = pick[moved]
    guard = moved & (size[target] == 1) & (size[curr] == 1) & (target > curr)
    target[guard] = curr[guard]
    return target, nwin >= 2


def replay(csr, trace, largest_label_wins=False):
    """Apply sweep_model to every oracle trace row's predecessor. Returns
    (rows, tied) stacked like `trace`."""
    nv = len(csr[0]) - 1
    rows, tied = [], []
    for k in range(len(trace)):
        curr = np.arange(nv, dtype=np.int64) if k == 0 else trace[k - 1]
        t, td = sweep_model(csr, curr, largest_label_wins)
        rows.append(t)
        tied.append(td)
    return np.array(rows), np.array(tied)


def oracle_run(csr, world=1, parts=None, trace_cap=64):
    """(mod, iters, target rows, per-iteration modularity) of the oracle on
    `csr` split `world` ways."""
    from oracle.oracle import OracleGraph, louvain
    nv = len(csr[0]) - 1
    parts = even_parts(nv, world) if parts is None else parts
    og = OracleGraph.from_csr(nv, world, parts, split(csr, parts))
    mod, iters, tt, tm = louvain(og, trace=True, trace_cap=trace_cap)
    og.free()
    assert iters < trace_cap, "oracle hit the trace cap"
    return mod, iters, tt.copy(), tm.copy()
