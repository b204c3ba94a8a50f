"""Host model of the multi-rank halo's exchange plan (numpy only), and the
tiny / lopsided inputs the halo tests run. Shared by test_halo_model_ref.py
(CPU, pins the inputs with the oracle alone) and test_gpu_halo_edges.py.

The model restates what the engine's halo does with the labels, from the
oracle's target trace, and returns exactly the fields of mv_halo_info:

 * Labels on the wire. Exchange 1 carries the identity, exchange k the
   oracle's target row k-1 (k = 2..K, K the iteration count). With the
   overlap there is one more exchange, carrying row K (the speculative one
   past the exit). Candidate discovery follows every exchange, on the same
   labels.
 * Segments. The segment b -> a is the sorted distinct tails of a's rows
   that b owns (a's ghosts at b, b's exports to a).
 * Arms. Per segment the sender remembers the labels last sent ("all
   changed" before exchange 1); `changed` counts the entries that differ.
   changed*12 >= seg*8 sends the whole segment (equality included), else
   changed > 0 sends (index, label) pairs, else nothing. Without delta
   compaction every non-empty segment goes whole.
 * Candidates. nrc of a rank = distinct labels outside [base, bound) among
   its own vertices' labels and its ghosts' labels; nreq = how many of the
   peers' candidates this rank owns.

All inputs are returned as (xadj, tails, w) with rows sorted by tail and
unit weights; the tests put ints123 on top.
"""
import numpy as np

from _multiphase_ref import clique, csr_from_edges, symmetric

FIELDS = ("exchanges",
          "send_full", "send_compact", "send_silent",
          "recv_full", "recv_compact", "recv_silent",
          "send_compact_entries", "recv_compact_entries",
          "prep_calls", "nrc_sum", "nrc_max", "nrc_zero", "nreq_sum")

ARM_FIELDS = ("full", "compact", "silent", "compact_entries")


def full_mode(changed, seg):
    """The whole segment is cheaper than, or as cheap as, the pairs (12 B
    per changed entry against 8 B per entry)."""
    return changed * 12 >= seg * 8


def ghosts_of(csr, parts):
    """Per rank: the sorted distinct remote tails of its rows."""
    xadj, tails, _ = csr
    out = []
    for lo, hi in zip(parts[:-1], parts[1:]):
        t = tails[xadj[lo]:xadj[hi]]
        out.append(np.unique(t[(t < lo) | (t >= hi)]))
    return out


def halo_model(csr, parts, trace, overlap, delta=True):
    """-> (per-rank list of {field: count} with the FIELDS of mv_halo_info,
    number of (pair, exchange) decisions that sat exactly on the equality
    edge changed*12 == seg*8)."""
    parts = np.asarray(parts, dtype=np.int64)
    p = len(parts) - 1
    nv = int(parts[-1])
    info = [dict.fromkeys(FIELDS, 0) for _ in range(p)]
    if p == 1:
        return info, 0
    trace = np.asarray(trace, dtype=np.int64)
    K = len(trace)
    wire = [np.arange(nv, dtype=np.int64)] + [trace[k] for k in range(K - 1)]
    if overlap:
        wire.append(trace[K - 1])
    ghosts = ghosts_of(csr, parts)
    segs = {}  # (sender b, receiver a) -> global ids, non-empty only
    for a in range(p):
        owner = np.searchsorted(parts, ghosts[a], "right") - 1
        for b in range(p):
            if b != a and np.any(owner == b):
                segs[(b, a)] = ghosts[a][owner == b]
    last = {key: np.full(seg.size, -1, dtype=np.int64)
            for key, seg in segs.items()}
    boundary = 0
    for lab in wire:
        for a in range(p):
            info[a]["exchanges"] += 1
        for (b, a), seg in segs.items():
            cur = lab[seg]
            if not delta:
                arm = "full"
            else:
                changed = int(np.sum(cur != last[(b, a)]))
                last[(b, a)] = cur.copy()
                if full_mode(changed, seg.size):
                    arm = "full"
                    boundary += changed * 12 == seg.size * 8
                elif changed > 0:
                    arm = "compact"
                    info[b]["send_compact_entries"] += changed
                    info[a]["recv_compact_entries"] += changed
                else:
                    arm = "silent"
            info[b]["send_" + arm] += 1
            info[a]["recv_" + arm] += 1
        cands = []
        for a in range(p):
            lo, hi = parts[a], parts[a + 1]
            vals = np.concatenate([lab[lo:hi], lab[ghosts[a]]])
            cands.append(np.unique(vals[(vals < lo) | (vals >= hi)]))
        for a in range(p):
            lo, hi = parts[a], parts[a + 1]
            nrc = int(cands[a].size)
            d = info[a]
            d["prep_calls"] += 1
            d["nrc_sum"] += nrc
            d["nrc_max"] = max(d["nrc_max"], nrc)
            d["nrc_zero"] += nrc == 0
            d["nreq_sum"] += sum(
                int(np.sum((cands[b] >= lo) & (cands[b] < hi)))
                for b in range(p) if b != a)
    return [{k: int(v) for k, v in d.items()} for d in info], int(boundary)


def arm_totals(info):
    """Send- and receive-side arm totals over the ranks:
    ({arm: count}, {arm: count}) for ARM_FIELDS."""
    send = {k: sum(d["send_" + k] for d in info) for k in ARM_FIELDS}
    recv = {k: sum(d["recv_" + k] for d in info) for k in ARM_FIELDS}
    return send, recv


# ---- inputs ----

def random_graph(seed, nv, ndraws=None, lo=0, hi=None):
    """`ndraws` (default 3*nv) random pairs among the vertices [lo, hi) of
    an nv-vertex graph, symmetrised; u == v draws are dropped, repeated
    pairs stay as parallel edges."""
    hi = nv if hi is None else hi
    rng = np.random.default_rng(seed)
    n = 3 * nv if ndraws is None else ndraws
    u = rng.integers(lo, hi, n)
    v = rng.integers(lo, hi, n)
    keep = u != v
    return symmetric(nv, u[keep], v[keep])


def random_parts(seed, nv, world):
    """Random cuts, every rank at least one vertex."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, nv), world - 1, replace=False))
    return np.concatenate([[0], cuts, [nv]]).astype(np.int64)


def one_per_rank():
    """nv 8: a ring with three chords, so every vertex has a neighbour and
    every neighbour is remote at one vertex per rank."""
    u = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 4])
    v = np.array([1, 2, 3, 4, 5, 6, 7, 0, 2, 3, 6])
    return symmetric(8, u, v)


def nine():
    """nv 9 for parts [0, 1, ..., 7, 9]: two triangles and a path."""
    u = np.array([0, 0, 1, 3, 3, 4, 2, 5, 6, 7, 8])
    v = np.array([1, 2, 2, 4, 5, 5, 3, 6, 7, 8, 0])
    return symmetric(9, u, v)


def chunk_edges():
    """nv 193 for parts [0, 1, 64, 128, 193]: lnv 1 | 63 | 64 | 65."""
    return random_graph(193, 193)


def isolated_tail():
    """nv 120: random pairs among vertices [0, 100); [100, 120) isolated."""
    return random_graph(120, 120, ndraws=300, hi=100)


def one_way():
    """nv 60 for parts [0, 30, 60]: a symmetric graph with every edge from
    rank 1 (rows >= 30) into rank 0 (tails < 30) removed, so only rank 0
    wants anything."""
    xadj, tails, w = random_graph(60, 60)
    src = np.repeat(np.arange(60, dtype=np.int64), np.diff(xadj))
    keep = ~((src >= 30) & (tails < 30))
    return csr_from_edges(60, src[keep], tails[keep], w[keep])


# name -> (generator, parts)
D1 = {
    "one_per_rank": (one_per_rank, list(range(9))),
    "nine_p8": (nine, list(range(8)) + [9]),
    "chunk_edges": (chunk_edges, [0, 1, 64, 128, 193]),
    "clique5_p5": (lambda: clique(5), [0, 1, 2, 3, 4, 5]),
    "clique5_p2": (lambda: clique(5), [0, 2, 5]),
    "isolated_tail": (isolated_tail, [0, 50, 100, 120]),
    "one_way": (one_way, [0, 30, 60]),
}

# (graph seed, nv, world): random_graph(seed, nv) cut by
# random_parts(seed, nv, world). Chosen by a seeded search for inputs on
# which the model reports every arm and the equality edge, under unit AND
# ints123 weights (test_halo_model_ref.py holds them to it).
D2 = {
    "arms_p2": (31, 34, 2),
    "arms_p3": (113, 34, 3),
    "arms_p4": (322, 38, 4),
}


def d2_input(name):
    seed, nv, world = D2[name]
    return random_graph(seed, nv), random_parts(seed, nv, world)
