"""GPU checks for the phase assignment, on-device community aggregation and
the multi-phase driver, against the host reference in _multiphase_ref.py
(numpy aggregation + the oracle once per phase; its own constants are
pinned by test_multiphase_ref.py).

Weight rule for an aggregated graph: offsets, tails and map exact; weights
exact when the fine weights are integer-valued, else within
(m-1) * 2^-52 * w of numpy's, m = fine edges in that run — the worst case
between two summation orders of m positive doubles (each order is within
(m-1) * 2^-53 relative of the true sum)."""
import functools
import json
import os

import numpy as np
import pytest

import _multiphase_ref as ref
from _coarsen_cases import (_assert_coarse_equal, _coarsen_case, _snap_equal,
                            _snapshot, _weights)
from _gpu_run import run_ranks

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pins.json")


def _graph(csr):
    from minivite_amd import Graph
    xadj, tails, w = csr
    nv = len(xadj) - 1
    return Graph.from_csr(nv, 0, 1, np.array([0, nv], dtype=np.int64), xadj,
                          tails, w)


# ---- 1. aggregation alone ----

COARSEN_CASES = ["nv1", "nv2", "nv63", "nv64", "nv65", "nv257", "no_edges",
                 "one_community", "identity_parallel", "sparse_unordered",
                 "isolated_and_loops", "community_of_1000", "parallel_5000",
                 "random_3000"]


@pytest.mark.parametrize("name", COARSEN_CASES)
def test_coarsen_csr_matches_numpy(name):
    from minivite_amd import coarsen_csr
    nv, u, v, comm = _coarsen_case(name)
    for mode in ("unit", "int", "real"):
        fine = ref.csr_from_edges(nv, u, v, _weights(mode, len(u), 5))
        g = _graph(fine)
        cg, cmap = coarsen_csr(g, comm)
        got = cg.arrays()
        assert cg.nv == cg.lnv == np.unique(comm).size
        cg.free()
        g.free()
        _assert_coarse_equal(got, fine, comm, cmap)


@pytest.mark.parametrize("name", ["random_3000", "parallel_5000",
                                  "community_of_1000"])
def test_coarsen_csr_is_deterministic(name):
    from minivite_amd import coarsen_csr
    nv, u, v, comm = _coarsen_case(name)
    g = _graph(ref.csr_from_edges(nv, u, v, _weights("real", len(u), 9)))
    outs = []
    for _ in range(2):
        cg, cmap = coarsen_csr(g, comm)
        outs.append(cg.arrays() + (cmap,))
        cg.free()
    g.free()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("bad", [-1, 6])
def test_coarsen_csr_rejects_out_of_range_labels(bad):
    from minivite_amd import coarsen_csr
    g = _graph(ref.clique(6))
    comm = np.arange(6)
    comm[3] = bad
    with pytest.raises(RuntimeError):
        coarsen_csr(g, comm)
    g.free()


# ---- shared oracle / engine runs ----

@functools.lru_cache(maxsize=None)
def _rgg_csr(unit):
    from oracle.oracle import OracleGraph
    og = OracleGraph.rgg(16384, 1, unit_weight=unit)
    csr = og.rank_arrays(0)
    og.free()
    return csr


def _engine_run(csr, trace_cap=256):
    """-> (mod, iters, trace rows, communities())."""
    from minivite_amd import Engine
    g = _graph(csr)
    e = Engine(device=0)
    e.load_graph(g)
    e.set_trace(trace_cap)
    mod, iters = e.run()
    tt, _ = e.trace(iters)
    tt = tt.copy()
    comm = e.communities()
    e.destroy()
    g.free()
    return mod, iters, tt, comm


# ---- 2. Engine.communities() ----

@pytest.mark.parametrize("unit", [True, False], ids=["unit", "w"])
def test_communities_is_trace_row_k_minus_3(unit):
    from oracle.oracle import OracleGraph, louvain
    csr = _rgg_csr(unit)
    og = OracleGraph.rgg(16384, 1, unit_weight=unit)
    _, oiters, ott, _ = louvain(og, trace=True)
    og.free()
    _, iters, _, comm = _engine_run(csr)
    assert iters == oiters >= 3
    assert np.array_equal(comm, ott[oiters - 3])


def test_communities_k2_branch_on_a_clique():
    _, iters, _, comm = _engine_run(ref.clique(5))
    assert iters == 2
    assert np.array_equal(comm, np.zeros(5, dtype=np.int64))


def test_communities_identity_without_edges():
    csr = (np.zeros(9, dtype=np.int64), np.zeros(0, dtype=np.int64),
           np.zeros(0))
    _, _, _, comm = _engine_run(csr, trace_cap=4)
    assert np.array_equal(comm, np.arange(8))


def test_communities_before_a_run_raises():
    from minivite_amd import Engine
    g = _graph(ref.clique(5))
    e = Engine(device=0)
    e.load_graph(g)
    with pytest.raises(RuntimeError):
        e.communities()
    e.destroy()
    g.free()


def test_communities_loopback_p2():
    from minivite_amd import Graph
    from oracle.oracle import OracleGraph, louvain
    nv, world = 16384, 2
    og = OracleGraph.rgg(nv, world)
    _, oiters, ott, _ = louvain(og, trace=True)
    og.free()

    def body(r, e):  # no trace armed
        g = Graph.rgg(nv, r, world)
        e.load_graph(g)
        _, iters = e.run()
        res = (iters, e.communities())
        g.free()
        return res

    results = run_ranks(world, body, join_s=600)
    assert results[0][0] == results[1][0] == oiters >= 3
    full = np.concatenate([results[r][1] for r in range(world)])
    assert np.array_equal(full, ott[oiters - 3])


# ---- 3. tiny graphs through the single-phase engine ----

def _tiny(name):
    if name == "nv1_selfloop":
        return ref.csr_from_edges(1, [0], [0], np.array([3.0]))
    if name == "nv2":
        return ref.csr_from_edges(2, [0, 1, 0], [1, 0, 0],
                                  np.array([2.0, 2.0, 1.0]))
    if name == "nv3":
        return ref.csr_from_edges(3, [0, 1, 1, 2, 2], [1, 0, 2, 1, 2],
                                  np.array([4.0, 4.0, 1.0, 1.0, 2.0]))
    if name == "clique5":
        return ref.clique(5)
    nv = int(name[2:])
    rng = np.random.default_rng(nv)
    u, v = rng.integers(0, nv, 3 * nv), rng.integers(0, nv, 3 * nv)
    w = rng.integers(1, 6, 3 * nv).astype(np.float64)
    keep = u != v
    loops = rng.integers(0, nv, 5)
    xadj, tails, wts = ref.symmetric(nv, u[keep], v[keep], w[keep])
    src = np.repeat(np.arange(nv), np.diff(xadj))
    return ref.csr_from_edges(nv, np.r_[src, loops], np.r_[tails, loops],
                              np.r_[wts, np.full(5, 2.0)])


@pytest.mark.parametrize("name", ["nv1_selfloop", "nv2", "nv3", "clique5",
                                  "nv63", "nv64", "nv65"])
def test_tiny_graph_single_phase_parity(name):
    from oracle.oracle import OracleGraph, louvain
    csr = _tiny(name)
    nv = len(csr[0]) - 1
    og = OracleGraph.from_csr(nv, 1, np.array([0, nv], dtype=np.int64),
                              [csr])
    omod, oiters, ott, _ = louvain(og, trace=True)
    og.free()
    mod, iters, tt, comm = _engine_run(csr)
    assert iters == oiters
    assert np.array_equal(tt, ott)
    assert abs(mod - omod) < 1e-9
    assert np.array_equal(comm, ref.phase_assignment(ott, oiters, nv))


# ---- 4. multi-phase, chained parity ----

MP_INPUTS = ["rgg_unit", "rgg_w", "ring30", "ring64", "clique5", "planted",
             "adv1", "adv2", "adv3"]
MP_CONSTANTS = {  # level sizes, iterations per phase (host reference)
    "rgg_unit": ([1956, 541, 167, 94, 89], [14, 8, 6, 4, 3, 2]),
    "ring30": ([30], [4, 3]),
    "ring64": ([64, 62, 32], [4, 3, 32, 2]),
}
THRESH = 1e-6


@functools.lru_cache(maxsize=None)
def _mp_input(name):
    if name == "rgg_unit":
        return _rgg_csr(True)
    if name == "rgg_w":
        return _rgg_csr(False)
    if name == "ring30":
        return ref.ring_of_cliques(30, 5)
    if name == "ring64":
        return ref.ring_of_cliques(64, 6)
    if name == "clique5":
        return ref.clique(5)
    if name == "planted":
        return ref.planted()
    return ref.adversarial(int(name[3:]))


def _run_mp(csr, max_phases=0, engine=None):
    from minivite_amd import Engine
    g = _graph(csr)
    e = engine or Engine(device=0)
    h = e.run_multiphase(g, thresh=THRESH, max_phases=max_phases)
    snap = _snapshot(h)
    h.free()
    if engine is None:
        e.destroy()
    g.free()
    return snap


@functools.lru_cache(maxsize=None)
def _mp_gpu(name):
    return _run_mp(_mp_input(name))


@pytest.mark.parametrize("name", MP_INPUTS)
def test_multiphase_chained_parity(name):
    csr0 = _mp_input(name)
    s = _mp_gpu(name)
    graphs = [csr0] + s["graphs"][1:]
    P, L = s["phases"], s["levels"]
    assert 1 <= P and L <= P
    assert abs(s["q"][0] - ref.level_modularity(*csr0)) < 1e-9
    for p in range(1, P + 1):
        info = s["info"][p]
        fine = graphs[p - 1]  # every phase before the last kept its level
        nv_in = len(fine[0]) - 1
        assert (info["nv_in"], info["ne_in"]) == (nv_in, len(fine[1]))
        omod, oiters, assign = ref.oracle_phase(*fine, thresh=THRESH)
        assert info["iters"] == oiters, f"phase {p}"                    # (a)
        assert abs(info["run_mod"] - omod) < 1e-9, f"phase {p}"         # (b)
        if p == 1 and np.all(csr0[2] == 1.0):  # unit: every sum is exact
            assert float(info["run_mod"]).hex() == float(omod).hex()
        omap, onc = ref.renumber(assign)
        assert info["nv_out"] == onc, f"phase {p}"
        if onc == nv_in:  # no merge: the run ends without a new level
            assert not info["kept"] and p == P and L == p - 1
            continue
        cx, ct, cw, _, _ = ref.coarsen(*fine, assign)
        q_new = ref.level_modularity(cx, ct, cw)
        assert abs(info["q_out"] - q_new) < 1e-9
        if not info["kept"]:  # dropped: q fell, and the run ends
            assert info["q_out"] < s["q"][p - 1] and p == P and L == p - 1
            continue
        assert L >= p
        assert np.array_equal(s["maps"][p], omap), f"phase {p}"         # (c)
        _assert_coarse_equal(graphs[p], fine, s["maps"][p])             # (d)
        assert abs(s["q"][p] - ref.level_modularity(*graphs[p])) < 1e-9  # (e)
        assert s["q"][p] >= s["q"][p - 1]
        gain = s["q"][p] - s["q"][p - 1]
        assert (p == P) == (gain < THRESH), f"phase {p}"
    # the whole run
    comm = np.arange(len(csr0[0]) - 1, dtype=np.int64)
    for k in range(1, L + 1):
        comm = s["maps"][k][comm]
    assert np.array_equal(s["communities"], comm)
    q_orig = ref.partition_modularity(*csr0, s["communities"])
    assert abs(q_orig - s["q"][L]) < 1e-9
    assert all(b >= a for a, b in zip(s["q"], s["q"][1:]))
    if name in MP_CONSTANTS:
        sizes, iters = MP_CONSTANTS[name]
        assert [len(g[0]) - 1 for g in graphs[1:]] == sizes
        assert [s["info"][p]["iters"] for p in range(1, P + 1)] == iters
    if name == "ring30":
        assert s["q"][1] == 0.8757575757575757
        assert s["info"][2]["nv_out"] == 28
    if name == "ring64":
        assert s["q"][L] == 0.93701171875
    if name == "clique5":
        assert s["q"][1] == 0.0 and s["info"][1]["iters"] == 2
        assert len(graphs[1][0]) - 1 == 1 and P == 2


# ---- 5. cap, hygiene and scope ----

def test_max_phases_one():
    from oracle.oracle import OracleGraph, louvain
    s = _run_mp(_rgg_csr(True), max_phases=1)
    assert s["phases"] == 1 and s["levels"] == 1
    og = OracleGraph.rgg(16384, 1)
    _, oiters, ott, _ = louvain(og, trace=True)
    og.free()
    omap, _ = ref.renumber(ref.phase_assignment(ott, oiters, 16384))
    assert np.array_equal(s["maps"][1], omap)
    assert np.array_equal(s["communities"], omap)


def test_engine_reuse_after_multiphase():
    """Two run_multiphase calls on one engine agree, and a reload + plain
    run afterwards reproduces the phase-one pin."""
    from minivite_amd import Graph, Engine
    from oracle.oracle import sha
    pin = json.load(open(GOLDEN))["rgg_n16384_p1_unit"]
    e = Engine(device=0)
    a = _run_mp(_rgg_csr(True), engine=e)
    b = _run_mp(_rgg_csr(True), engine=e)
    assert _snap_equal(a, b)
    assert _snap_equal(a, _mp_gpu("rgg_unit"))
    g = Graph.rgg(16384, 0, 1)
    e.load_graph(g)
    e.set_trace(64)
    mod, iters = e.run()
    tt, _ = e.trace(iters)
    assert iters == pin["iters"]
    assert float(mod).hex() == pin["final_mod_hex"]
    assert [sha(tt[k]) for k in range(iters)] == pin["iter_target_sha"]
    e.destroy()
    g.free()


def test_multiphase_refuses_multi_rank():
    """The rank-count check comes before any load or exchange, so one
    rank of a two-rank loopback session raises on its own."""
    from minivite_amd import Graph, Engine, LoopbackSession
    ses = LoopbackSession(2)
    e = Engine.loopback(ses, 0, device=0)
    g = Graph.rgg(16384, 0, 2)
    with pytest.raises(RuntimeError):
        e.run_multiphase(g)
    e.destroy()
    g.free()
    ses.destroy()


# ---- 6. CLI ----

def test_cli_multiphase_and_community_file(tmp_path):
    import re
    import subprocess
    cli = os.path.join(REPO, "minivite_amd", "mv355")
    out_m = tmp_path / "multi.txt"
    r = subprocess.run([cli, "-n", "16384", "-l", "-m", "-o", str(out_m)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Modularity, #Iterations: 0.752138, 14" in r.stdout
    outs = [int(m) for m in re.findall(r"^Phase \d+:.* vertices out (\d+)",
                                       r.stdout, re.M)]
    assert outs == [1956, 541, 167, 94, 89], r.stdout
    assert re.search(r"^Communities, q: 89, 0\.96672369", r.stdout, re.M)
    comm = np.loadtxt(out_m, dtype=np.int64)
    assert comm.shape == (16384,) and np.unique(comm).size == 89

    out_1 = tmp_path / "single.txt"
    r = subprocess.run([cli, "-n", "16384", "-l", "-o", str(out_1)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Phase" not in r.stdout
    comm = np.loadtxt(out_1, dtype=np.int64)
    assert comm.shape == (16384,) and np.unique(comm).size == 1956

    r = subprocess.run([cli, "-n", "16384", "-l", "-m", "-g", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "single-GPU" in r.stderr
