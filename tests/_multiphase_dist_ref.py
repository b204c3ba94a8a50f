"""Host model of the multi-phase driver across ranks. Shared by
test_multiphase_dist_ref.py (CPU, pins the yardstick) and
test_gpu_multiphase_dist.py.

The model is _multiphase_ref.run_multiphase with a partition per level:
every phase runs the oracle on the current level split by that level's
`parts`, the assignment is aggregated on the STITCHED level (the coarse
graph of a partitioned level is defined as the coarse graph of the stitched
one), and the next level is split evenly (_tie_graphs.even_parts), so a
level with fewer vertices than ranks leaves some ranks without vertices.

coarse_weights_two_stage is the summation order of the distributed
aggregation in numpy: every rank reduces its own edges per coarse pair,
the owner then adds the per-rank partials in ascending rank order.
"""
import functools

import numpy as np

import _halo_model as hm
import _multiphase_ref as ref
import _tie_graphs as tg
from oracle.oracle import OracleGraph, louvain

THRESH = 1e-6
RANDOM_PARTS_SEED = 5

# level sizes, iterations per phase, final q of the single-rank reference;
# exact=False: real weights, q compared to 1e-9
TABLE = {
    "ring30": ([30], [4, 3], 0.8757575757575757, True),
    "ring64": ([64, 62, 32], [4, 3, 32, 2], 0.93701171875, True),
    "clique5": ([1], [2, 2], 0.0, True),
    "planted": ([41, 40], [16, 3, 2], 0.8277247318290912, True),
    "adv3": ([1738, 959, 602, 475, 441], [4, 5, 6, 5, 3, 3],
             0.5822581736660452, True),
    "adv4": ([777, 403, 353, 320, 311, 307], [8, 6, 3, 4, 3, 3, 2],
             0.2443817501980504, False),
    "rgg_unit": ([1956, 541, 167, 94, 89], [14, 8, 6, 4, 3, 2],
                 0.9667236972707427, True),
    "rgg_w": ([1389, 386, 129, 91, 85, 84], [16, 8, 6, 3, 4, 3, 2],
              0.9630189305189122, False),
}


@functools.lru_cache(maxsize=None)
def mp_input(name):
    """The CSR of a TABLE input; built once, read-only."""
    if name in ("rgg_unit", "rgg_w"):
        og = OracleGraph.rgg(16384, 1, unit_weight=name == "rgg_unit")
        csr = og.rank_arrays(0)
        og.free()
        return csr
    if name == "ring30":
        return ref.ring_of_cliques(30, 5)
    if name == "ring64":
        return ref.ring_of_cliques(64, 6)
    if name == "clique5":
        return ref.clique(5)
    if name == "planted":
        return ref.planted()
    return ref.adversarial(int(name[3:]))


def parts_of(kind, nv, world):
    if kind == "even" or world == 1:
        return tg.even_parts(nv, world)
    return hm.random_parts(RANDOM_PARTS_SEED, nv, world)


def oracle_phase(csr, parts, thresh=THRESH):
    """One oracle run on `csr` split by `parts` -> (run_mod, iters,
    assignment)."""
    nv = len(csr[0]) - 1
    parts = np.asarray(parts, dtype=np.int64)
    og = OracleGraph.from_csr(nv, len(parts) - 1, parts, tg.split(csr, parts))
    mod, iters, tt, _ = louvain(og, thresh=thresh, trace=True, trace_cap=256)
    og.free()
    assert iters < 256, "oracle hit the trace cap"
    return mod, iters, ref.phase_assignment(tt, iters, nv)


def run_multiphase_dist(csr, parts0, thresh=THRESH, max_phases=0):
    """The driver rule across len(parts0)-1 ranks. The dict of
    _multiphase_ref.run_multiphase plus parts[k] for k = 0..L."""
    world = len(parts0) - 1
    cap = max_phases if max_phases >= 1 else ref.MAX_PHASES
    graphs = [csr]
    parts = [np.asarray(parts0, dtype=np.int64)]
    maps = [None]
    q = [ref.level_modularity(*csr)]
    phases = []
    for _ in range(cap):
        fine = graphs[-1]
        nv = len(fine[0]) - 1
        mod, iters, assign = oracle_phase(fine, parts[-1], thresh)
        info = dict(iters=iters, run_mod=mod, nv_in=nv, nv_out=nv,
                    q_out=q[-1], kept=False)
        phases.append(info)
        if np.unique(assign).size == nv:
            break
        nx, nt, nw, cmap, _ = ref.coarsen(*fine, assign)
        qn = ref.level_modularity(nx, nt, nw)
        info["nv_out"], info["q_out"] = len(nx) - 1, qn
        if qn < q[-1]:
            break
        info["kept"] = True
        gain = qn - q[-1]
        graphs.append((nx, nt, nw))
        parts.append(tg.even_parts(len(nx) - 1, world))
        maps.append(cmap)
        q.append(qn)
        if gain < thresh:
            break
    comm = np.arange(len(csr[0]) - 1, dtype=np.int64)
    for cmap in maps[1:]:
        comm = cmap[comm]
    return dict(graphs=graphs, parts=parts, maps=maps, q=q, phases=phases,
                communities=comm)


def summary(h):
    return ([len(g[0]) - 1 for g in h["graphs"][1:]],
            [p["iters"] for p in h["phases"]])


def coarse_weights_two_stage(csr, parts, comm):
    """Weights of ref.coarsen(csr, comm), in its order, summed the
    distributed way: per rank over its own rows (reduceat over the rank's
    stably sorted keys), then the partials of a pair in rank order."""
    xadj, tails, w = csr
    cmap, nc = ref.renumber(np.asarray(comm, dtype=np.int64))
    pk, pw = [], []
    for r, (xa, ta, wa) in enumerate(tg.split(csr, parts)):
        src = np.repeat(np.arange(len(xa) - 1, dtype=np.int64) + parts[r],
                        np.diff(xa))
        key = cmap[src] * nc + cmap[ta]
        order = np.argsort(key, kind="stable")
        ks, ws = key[order], wa[order]
        if ks.size == 0:
            continue
        heads = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        pk.append(ks[heads])
        pw.append(np.add.reduceat(ws, heads))
    if not pk:
        return np.zeros(0)
    keys, partial = np.concatenate(pk), np.concatenate(pw)
    order = np.argsort(keys, kind="stable")  # equal keys stay in rank order
    keys, partial = keys[order], partial[order]
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    ends = np.r_[heads[1:], keys.size]
    out = np.zeros(heads.size)
    for k in range(len(parts) - 1):  # left to right: ascending rank
        idx = heads + k
        live = idx < ends
        out[live] += partial[idx[live]]
    return out
