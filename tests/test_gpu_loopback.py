"""Multi-rank HIP path on ONE GPU via the loopback transport.

RCCL refuses two ranks on one device, so the p>1 engine code — the
view-mode K4 sweeps (the MR=true instantiations of sweep.hip's k4_sweep /
k4_sweep_iter1 / k4_sweep_hi, and k4_sweep_lh), k8 community gathers, view builds, candidate filter +
sort/unique, K9 replies, delta compaction, per-sender delta application,
and the whole deep-pipelined per-iteration exchange protocol
(dspl.hpp:497-1103 equivalents) — is executed here with the collectives
replaced by device-to-device copies + host barriers (mv_lb_session).
Every kernel and every byte layout is the production p>1 path; only
ncclSend/Recv itself is substituted. Parity: bit-exact vs the
reference-pinned oracle fixtures (tests/golden/pins.json) or the oracle
on identical partitioned inputs.
"""
import json
import os

import numpy as np
import pytest

import _tie_graphs as tg
from _gpu_run import (GOLDEN, by_run, check_vs_oracle, check_vs_pin, knobs,
                      run_csrs, run_ranks, run_rgg, traced_run)

pytestmark = pytest.mark.gpu


def _pin(key):
    return json.load(open(GOLDEN))[key]


@pytest.mark.parametrize("world", [2, 4, 8])
def test_loopback_parity_unit(world):
    check_vs_pin(run_rgg(16384, world), _pin(f"rgg_n16384_p{world}_unit"))


def test_loopback_parity_p8_n32768():
    """The round-end 8-GPU topology's pin at a larger graph."""
    check_vs_pin(run_rgg(32768, 8), _pin("rgg_n32768_p8_unit"))


def _run_sequence(world, loads, runs_per_load=1):
    """One engine per rank, kept alive across `loads` (a list of RGG sizes,
    each loaded in turn on the SAME engine) with `runs_per_load` runs after
    every load -> one {rank: record} per run."""
    from minivite_amd import Graph

    def body(r, e):
        recs = []
        for nv in loads:
            g = Graph.rgg(nv, r, world, unit_weight=True)
            recs += traced_run(e, g, nruns=runs_per_load)
            g.free()
        return recs

    return by_run(run_ranks(world, body, join_s=600))


def test_loopback_rerun_p2():
    """Two run() calls on the same loaded engines (p=2): the second run
    reuses the ghost / export / delta buffers the first one sized and must
    re-initialise them (last-sent labels back to "all changed"), so both
    runs match the pin bit-for-bit."""
    pin = _pin("rgg_n16384_p2_unit")
    for records in _run_sequence(2, [16384], runs_per_load=2):
        check_vs_pin(records, pin)


def test_loopback_reload_grow_shrink_p4():
    """load_graph on live engines (p=4): a larger graph, then the first
    one again. Every per-graph buffer and size must follow the load -- no
    stale capacity, ghost count or trace buffer from the previous graph."""
    sizes = [16384, 65536, 16384]
    for nv, records in zip(sizes, _run_sequence(4, sizes)):
        check_vs_pin(records, _pin(f"rgg_n{nv}_p4_unit"))


def test_loopback_parity_weighted_p2():
    """-w path at p=2: communities bit-exact, modularity < 1e-9 (the
    reference's own cross-thread accumulation granularity)."""
    check_vs_pin(run_rgg(16384, 2, unit=False), _pin("rgg_n16384_p2_w"),
                 exact_mod=False)


def test_loopback_parity_no_overlap_p4():
    """The non-overlapped halo path (MV_NO_OVERLAP) must produce the same
    bits -- overlap is pure scheduling."""
    with knobs(MV_NO_OVERLAP="1"):
        records = run_rgg(16384, 4)
    check_vs_pin(records, _pin("rgg_n16384_p4_unit"))


def test_loopback_parity_no_delta_p4():
    """Full-resend #1a (MV_NO_DELTA, the reference's wire behavior) must
    produce the same bits as the delta-compacted default."""
    with knobs(MV_NO_DELTA="1"):
        records = run_rgg(16384, 4)
    check_vs_pin(records, _pin("rgg_n16384_p4_unit"))


def _zipf_graph(nv, max_deg, seed=7, weighted=False):
    rng = np.random.default_rng(seed)
    deg = np.minimum((2.0 / rng.power(2.0, nv)).astype(np.int64), max_deg)
    src = np.repeat(np.arange(nv), deg)
    dst = rng.integers(0, nv, src.size)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    u = np.concatenate([src, dst])
    v = np.concatenate([dst, src])
    if weighted:
        w0 = rng.uniform(0.01, 1.0, src.size)
        w = np.concatenate([w0, w0])
    else:
        w = None
    order = np.lexsort((v, u))
    u, v = u[order], v[order]
    if w is not None:
        w = w[order]
    xadj = np.zeros(nv + 1, dtype=np.int64)
    np.add.at(xadj, u + 1, 1)
    xadj = np.cumsum(xadj)
    return xadj, v, w


@pytest.mark.parametrize("weighted", [False, True])
def test_loopback_skewed_p2(weighted):
    """Skewed (hub-heavy) graph partitioned 2 ways: exercises the
    multi-rank wave-per-vertex hub kernel (unit) / the spill path (-w)
    under the view encoding; engine vs oracle on identical CSRs. Each
    rank runs twice on the same engine: the second run rebuilds the
    hash-band offsets and reuses the band buffers."""
    nv, world = 50000, 2
    xadj, tails, w = _zipf_graph(nv, 5000, weighted=weighted)
    parts = np.array([(nv * r) // world for r in range(world + 1)],
                     dtype=np.int64)
    csrs = tg.split((xadj, tails, w), parts)
    oracle = _oracle(nv, parts, csrs, trace_cap=300)
    runs = run_csrs(csrs, parts, trace_cap=300, nruns=2, join_s=600)
    for records in runs:
        check_vs_oracle(records, oracle, parts, exact_mod=not weighted)


def test_loopback_balanced_read_p4():
    """-b edge-balanced reader (find_balanced_num_edges partition,
    graph.hpp:416-461) feeding the ENGINE at p=4 on one GPU: engine vs
    oracle on the identical balanced partition of the same .bin."""
    import tempfile
    from minivite_amd import Graph, lib
    from oracle.oracle import OracleGraph, louvain
    nv, world = 16384, 4
    g0 = Graph.rgg(nv, 0, 1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "g.bin")
        g0.write_binary(path)
        g0.free()
        graphs, parts = [], None
        for r in range(world):
            gr = Graph.read_binary(path, r, world, balanced=True)
            if parts is None:
                pp = lib().mv_graph_parts(gr.h)
                parts = np.array([pp[k] for k in range(world + 1)],
                                 dtype=np.int64)
            graphs.append(gr)
        og = OracleGraph.from_csr(nv, world, parts,
                                  [g.arrays() for g in graphs])
        oracle = louvain(og, trace=True)
        og.free()
        records = run_ranks(world,
                            lambda r, e: traced_run(e, graphs[r])[0],
                            join_s=600)
        for g in graphs:
            g.free()
    check_vs_oracle(records, oracle, parts)


def _oracle(nv, parts, csrs, trace_cap):
    from oracle.oracle import OracleGraph, louvain
    og = OracleGraph.from_csr(nv, len(parts) - 1, parts, csrs)
    result = louvain(og, trace=True, trace_cap=trace_cap)
    og.free()
    return result


def _loopback_vs_oracle(nv, world, csrs, parts, trace_cap=64,
                        exact_mod=True):
    """Run `world` loopback engines on the given per-rank CSRs and compare
    per-iteration targets + modularity against the oracle on the same
    partition."""
    records, = run_csrs(csrs, parts, trace_cap, join_s=900)
    check_vs_oracle(records, _oracle(nv, parts, csrs, trace_cap), parts,
                    exact_mod)


def test_loopback_large_p4_n1048576():
    """n=2^20 RGG at p=4 through the engines: larger ghost sets, multi-
    chunk SELL, grid-stride sweeps and realloc-growth paths under the
    pipelined halo (the pins only cover n<=32768)."""
    from minivite_amd import Graph
    nv, world = 1 << 20, 4
    parts = np.array([(nv * r) // world for r in range(world + 1)],
                     dtype=np.int64)
    csrs = []
    for r in range(world):
        g = Graph.rgg(nv, r, world)
        csrs.append(g.arrays())
        g.free()
    _loopback_vs_oracle(nv, world, csrs, parts)


def test_loopback_random_edges_p4():
    """configs[3]-shaped input: RGG + 4% random long-range edges at p=4 —
    stresses alltoallv volume and the delta-compaction full/compact mix."""
    from minivite_amd import Graph
    nv, world = 65536, 4
    parts = np.array([(nv * r) // world for r in range(world + 1)],
                     dtype=np.int64)
    csrs = []
    for r in range(world):
        g = Graph.rgg(nv, r, world, random_edge_percent=4.0)
        csrs.append(g.arrays())
        g.free()
    _loopback_vs_oracle(nv, world, csrs, parts)


def test_loopback_p3_nonpow2():
    """Non-power-of-two rank count (the reference accepts any nprocs for
    -f inputs): p=3 engines on a random flat graph."""
    rng = np.random.default_rng(23)
    nv, world = 30000, 3
    m = nv * 5
    u = rng.integers(0, nv, m)
    v = rng.integers(0, nv, m)
    uu = np.concatenate([u, v])
    vv = np.concatenate([v, u])
    order = np.lexsort((vv, uu))
    uu, vv = uu[order], vv[order]
    xadj = np.zeros(nv + 1, dtype=np.int64)
    np.add.at(xadj, uu + 1, 1)
    xadj = np.cumsum(xadj)
    parts = np.array([0, 9000, 21000, 30000], dtype=np.int64)
    _loopback_vs_oracle(nv, world, tg.split((xadj, vv, None), parts), parts,
                        trace_cap=256)


@pytest.mark.parametrize("trial", [0, 1, 2, 3, 4])
def test_loopback_fuzz(trial):
    """Randomized small graphs (self-loops, parallel edges, isolated
    vertices, mixed weights) x rank counts {2,3,4,6,8}: the multi-rank
    engine must match the oracle bit-for-bit on arbitrary partitioned
    inputs."""
    rng = np.random.default_rng(1000 + trial)
    nv = int(rng.integers(2000, 8000))
    world = [2, 3, 4, 6, 8][trial]
    unit = trial not in (1, 3)
    m = nv * int(rng.integers(3, 9))
    u = rng.integers(0, nv, m)
    v = rng.integers(0, nv, m)
    loops = rng.integers(0, nv, max(nv // 30, 1))
    uu = np.concatenate([u, v, loops, u[:m // 5]])
    vv = np.concatenate([v, u, loops, v[:m // 5]])
    if unit:
        w = None
    else:
        w = rng.uniform(0.01, 1.0, uu.size)
    order = np.lexsort((vv, uu))
    uu, vv = uu[order], vv[order]
    if w is not None:
        w = w[order]
    xadj = np.zeros(nv + 1, dtype=np.int64)
    np.add.at(xadj, uu + 1, 1)
    xadj = np.cumsum(xadj)
    cuts = np.sort(rng.choice(np.arange(1, nv), world - 1, replace=False))
    parts = np.concatenate([[0], cuts, [nv]]).astype(np.int64)
    _loopback_vs_oracle(nv, world, tg.split((xadj, vv, w), parts), parts,
                        trace_cap=256, exact_mod=unit)


def test_loopback_deterministic_p4():
    """Two identical p=4 loopback runs agree bit-for-bit (per-sender
    in-order delta application — run-to-run determinism at nranks > 2)."""
    r1 = run_rgg(16384, 4)
    r2 = run_rgg(16384, 4)
    for r in range(4):
        assert float(r1[r]["mod"]).hex() == float(r2[r]["mod"]).hex()
        assert r1[r]["iters"] == r2[r]["iters"]
        assert np.array_equal(r1[r]["targets"], r2[r]["targets"])
