"""The hand-built input of the sweep row-chain tests. Shared by
test_sweep_chain_inputs_ref.py (CPU, pins it with the oracle alone) and
test_gpu_sweep_chain.py.

The graph is a disjoint union, in label order:

 * a degree ladder: for every d in LADDER one hub joined to d leaves of its
   own, so the hub has degree d and the leaves degree 1 (a chunk of the edge
   loop holds 8 steps: 7, 8, 9 and 15, 16, 17 sit on either side of one and
   of two chunks);
 * one vertex with a self-loop and two leaves;
 * a planted partition, which keeps the run alive for several iterations
   while the rest is swept again in each, and whose vertices of degree >= 9
   still move after iteration 2. It is sized so that the graph has 64 rows
   of 64 positions (65 at rem 1): with units of three rows and one block of
   four waves, 18 of the 22 units are handed out by the row queue;
 * isolated vertices, at least ISOLATED_MIN of them. The engine sorts a
   graph without a locality hint by descending degree, so they fill the end
   of the SELL image: with 127 or more of them one whole slice of 64
   positions has width 0 wherever the slices fall. Their number is chosen so
   that nv is `rem` modulo 64.

Rows are sorted by tail. Weights are unit; _tie_graphs.ints123 puts integer
weights 1..3 on top.
"""
import numpy as np

from _multiphase_ref import csr_from_edges, planted
from _tie_graphs import union

LADDER = (7, 8, 9, 15, 16, 17)
ISOLATED_MIN = 130
PLANTED = dict(seed=12, nblocks=96, bsize=40, npairs=19200)


def _ladder():
    u, v, base = [], [], 0
    for d in LADDER:
        leaves = base + 1 + np.arange(d)
        u.append(np.full(d, base))
        v.append(leaves)
        base += d + 1
    # the self-loop vertex: one (z, z) entry and two leaves
    z = base
    u.append(np.array([z, z, z]))
    v.append(np.array([z, z + 1, z + 2]))
    base += 3
    u, v = np.concatenate(u), np.concatenate(v)
    keep = u != v  # the loop is stored once, every other pair both ways
    return csr_from_edges(base, np.concatenate([u, v[keep]]),
                          np.concatenate([v, u[keep]]))


def chain_graph(rem):
    """(xadj, tails, w) with nv % 64 == rem."""
    core = union(_ladder(), planted(**PLANTED))
    nv = len(core[0]) - 1
    iso = ISOLATED_MIN + (rem - (nv + ISOLATED_MIN)) % 64
    xadj = np.concatenate([core[0], np.full(iso, core[0][-1])])
    return xadj, core[1], core[2]


def self_loop_vertex():
    return sum(d + 1 for d in LADDER)
