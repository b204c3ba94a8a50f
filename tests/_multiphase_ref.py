"""Host reference for the multi-phase driver: numpy community aggregation
plus a driver that runs the oracle once per phase. Shared by
test_multiphase_ref.py (CPU, pins the yardstick) and test_gpu_multiphase.py.

Definitions (multi-phase section):
 * phase assignment of a K-iteration run = trace row K-3 (K >= 3), row 0
   (K == 2), the identity (K == 1);
 * coarse graph = every directed fine edge (u, v, w) adds w to
   (C(u), C(v)), C(u) == C(v) included; labels renumbered dense in
   ascending order; one CSR entry per distinct pair, tails ascending;
 * q(level) = sum_c selfloop_c / W - sum_c deg_c^2 / W^2.
"""
import numpy as np

from oracle.oracle import OracleGraph, louvain

MAX_PHASES = 64  # the driver's safety bound when max_phases < 1


# ---- graph builders (CSR with rows sorted by tail) ----

def csr_from_edges(nv, u, v, w=None):
    """Directed edge list -> (xadj, tails, weights); parallel edges stay."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    w = np.ones(u.size) if w is None else np.asarray(w, dtype=np.float64)
    order = np.lexsort((v, u))
    u, v, w = u[order], v[order], w[order]
    xadj = np.zeros(nv + 1, dtype=np.int64)
    np.add.at(xadj, u + 1, 1)
    return np.cumsum(xadj), v.copy(), w.copy()


def symmetric(nv, u, v, w=None):
    """Undirected pairs -> CSR storing each pair in both directions."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    ww = None if w is None else np.concatenate([w, w])
    return csr_from_edges(nv, np.concatenate([u, v]), np.concatenate([v, u]),
                          ww)


def clique(k):
    u, v = np.triu_indices(k, 1)
    return symmetric(k, u, v)


def ring_of_cliques(ncliques, k):
    """Clique i = vertices [i*k, (i+1)*k); the last vertex of clique i is
    joined to the first vertex of clique i+1 (cyclically). Unit weights."""
    iu, iv = np.triu_indices(k, 1)
    base = np.arange(ncliques)[:, None] * k
    u = (base + iu[None, :]).ravel()
    v = (base + iv[None, :]).ravel()
    last = np.arange(ncliques) * k + (k - 1)
    first = ((np.arange(ncliques) + 1) % ncliques) * k
    return symmetric(ncliques * k, np.concatenate([u, last]),
                     np.concatenate([v, first]))


def planted(seed=11, nblocks=40, bsize=50, npairs=30000, p_in=0.85):
    """Planted partition: npairs sampled pairs, p_in of them in-block,
    symmetrised; duplicates stay as parallel edges, u == v pairs dropped."""
    rng = np.random.default_rng(seed)
    nv = nblocks * bsize
    inside = rng.random(npairs) < p_in
    u = rng.integers(0, nv, npairs)
    v_in = (u // bsize) * bsize + rng.integers(0, bsize, npairs)
    v_out = rng.integers(0, nv, npairs)
    v = np.where(inside, v_in, v_out)
    keep = u != v
    return symmetric(nv, u[keep], v[keep])


def adversarial(seed):
    """The generator pattern of test_adversarial_graphs_parity: self-loops,
    parallel edges, isolated vertices; odd seeds unit, even seeds real
    weights."""
    rng = np.random.default_rng(seed)
    nv = int(rng.integers(500, 4000))
    unit = bool(seed % 2)
    m = nv * int(rng.integers(2, 8))
    u = rng.integers(0, nv, m)
    v = rng.integers(0, nv, m)
    selfloops = rng.integers(0, nv, max(nv // 20, 1))
    u = np.concatenate([u, v, selfloops])
    v = np.concatenate([v, u[:m], selfloops])
    u = np.concatenate([u, u[:m // 4]])
    v = np.concatenate([v, v[:m // 4]])
    w = np.ones(u.size) if unit else rng.uniform(0.01, 1.0, u.size)
    dead = rng.integers(0, nv, max(nv // 10, 1))
    keep = ~(np.isin(u, dead) | np.isin(v, dead))
    return csr_from_edges(nv, u[keep], v[keep], w[keep])


# ---- the definitions ----

def renumber(comm):
    """Dense ids in ascending label order -> (map, nc)."""
    labels = np.unique(comm)
    return np.searchsorted(labels, comm).astype(np.int64), int(labels.size)


def coarsen(xadj, tails, w, comm):
    """-> (cxadj, ctails, cweights, map, run_lengths)."""
    nv = len(xadj) - 1
    cmap, nc = renumber(np.asarray(comm, dtype=np.int64))
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(xadj))
    key = cmap[src] * nc + cmap[tails]
    order = np.argsort(key, kind="stable")
    ks, ws = key[order], np.asarray(w, dtype=np.float64)[order]
    cxadj = np.zeros(nc + 1, dtype=np.int64)
    if ks.size == 0:
        return (cxadj, np.zeros(0, np.int64), np.zeros(0), cmap,
                np.zeros(0, np.int64))
    heads = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    runs = np.diff(np.r_[heads, ks.size])
    cw = np.add.reduceat(ws, heads)
    np.add.at(cxadj, ks[heads] // nc + 1, 1)
    return np.cumsum(cxadj), ks[heads] % nc, cw, cmap, runs


def level_modularity(xadj, tails, w):
    """q of a level's graph (each vertex = one community of the original)."""
    nv = len(xadj) - 1
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(xadj))
    W = float(np.sum(w))
    if W == 0.0:
        return 0.0
    deg = np.bincount(src, weights=w, minlength=nv)
    loops = float(np.sum(w[src == tails]))
    return loops / W - float(np.sum(deg * deg)) / (W * W)


def partition_modularity(xadj, tails, w, comm):
    """Modularity of `comm` on the graph itself (same formula, no coarse
    graph built)."""
    nv = len(xadj) - 1
    cmap, nc = renumber(np.asarray(comm, dtype=np.int64))
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(xadj))
    W = float(np.sum(w))
    if W == 0.0:
        return 0.0
    deg = np.bincount(cmap[src], weights=w, minlength=nc)
    e_in = float(np.sum(w[cmap[src] == cmap[tails]]))
    return e_in / W - float(np.sum(deg * deg)) / (W * W)


def phase_assignment(trace, iters, nv):
    if iters >= 3:
        return trace[iters - 3].copy()
    if iters == 2:
        return trace[0].copy()
    return np.arange(nv, dtype=np.int64)


def oracle_phase(xadj, tails, w, thresh=1e-6):
    """One oracle run -> (run_mod, iters, assignment)."""
    nv = len(xadj) - 1
    og = OracleGraph.from_csr(nv, 1, np.array([0, nv], dtype=np.int64),
                              [(xadj, tails, w)])
    mod, iters, tt, _ = louvain(og, thresh=thresh, trace=True, trace_cap=256)
    og.free()
    assert iters < 256, "oracle hit the trace cap"
    return mod, iters, phase_assignment(tt, iters, nv)


def run_multiphase(xadj, tails, w, thresh=1e-6, max_phases=0):
    """The driver rule. Returns a dict:
    graphs[k] (k = 0..L), maps[k] (k = 1..L, index 0 unused), q[k],
    phases = [dict(iters, run_mod, nv_in, nv_out, q_out, kept)],
    communities (nv0 dense ids)."""
    cap = max_phases if max_phases >= 1 else MAX_PHASES
    graphs = [(xadj, tails, w)]
    maps = [None]
    q = [level_modularity(xadj, tails, w)]
    phases = []
    for _ in range(cap):
        cx, ct, cw = graphs[-1]
        nv = len(cx) - 1
        mod, iters, assign = oracle_phase(cx, ct, cw, thresh)
        info = dict(iters=iters, run_mod=mod, nv_in=nv, nv_out=nv,
                    q_out=q[-1], kept=False)
        phases.append(info)
        if np.unique(assign).size == nv:
            break
        nx, nt, nw, cmap, _ = coarsen(cx, ct, cw, assign)
        qn = level_modularity(nx, nt, nw)
        info["nv_out"], info["q_out"] = len(nx) - 1, qn
        if qn < q[-1]:
            break
        info["kept"] = True
        gain = qn - q[-1]
        graphs.append((nx, nt, nw))
        maps.append(cmap)
        q.append(qn)
        if gain < thresh:
            break
    comm = np.arange(len(xadj) - 1, dtype=np.int64)
    for cmap in maps[1:]:
        comm = cmap[comm]
    return dict(graphs=graphs, maps=maps, q=q, phases=phases,
                communities=comm)
