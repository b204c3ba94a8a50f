"""GPU checks for multi-phase Louvain across ranks: slices without
vertices through the single-phase engine (G1), the distributed aggregation
alone (G2), the distributed driver against the host model of
_multiphase_dist_ref.py (G3), its degenerate and hygiene cases (G4) and
one run over real RCCL (G5, needs two devices).

Ranks are loopback engines on device 0, one daemon thread per rank
(_gpu_run.run_ranks); a thread still alive after the join timeout ends the
pytest session, so mismatched collectives cannot wedge it.

Weight rule for an aggregated graph, as in test_gpu_multiphase.py: offsets,
tails, map and parts exact; weights exact when the fine weights are
integer-valued, else within (m-1) * 2^-52 * w of numpy's, m = global fine
edges of that run -- the bound between any two summation orders of m
positive doubles, the two-stage order (per rank, then rank order)
included."""
import functools
import json

import numpy as np
import pytest

import _multiphase_dist_ref as dref
import _multiphase_ref as ref
import _tie_graphs as tg
from _coarsen_cases import (_assert_coarse_equal, _coarsen_case, _snap_equal,
                            _snapshot, _weights)
from _gpu_run import (GOLDEN, check_vs_oracle, check_vs_pin, run_csrs,
                      run_ranks, traced_run)

pytestmark = pytest.mark.gpu

THRESH = dref.THRESH
TRACE_CAP = 64
JOIN_S = 120


# ---- running ----

def _run_ranks(world, body):
    return run_ranks(world, body, join_s=JOIN_S)


def _slice(csr, parts, r):
    from minivite_amd import Graph
    xa, ta, wa = tg.split(csr, parts)[r]
    return Graph.from_csr(int(parts[-1]), r, len(parts) - 1, parts, xa, ta,
                          wa)


def _stitch(slices):
    """Per-rank (xadj, tails, w) in rank order -> the whole CSR."""
    xadj, off = [np.zeros(1, dtype=np.int64)], 0
    for xa, _, _ in slices:
        xadj.append(xa[1:] + off)  # empty for a rank without vertices
        off += xa[-1]
    return (np.concatenate(xadj), np.concatenate([s[1] for s in slices]),
            np.concatenate([s[2] for s in slices]))


# ---- G1: slices without vertices, single phase ----

EMPTY_PARTS = {"tail": [0, 24, 24], "head": [0, 0, 24],
               "middle": [0, 3, 3, 24]}


@pytest.mark.parametrize("weights", ["unit", "ints123"])
@pytest.mark.parametrize("name", list(EMPTY_PARTS))
def test_empty_slice_single_phase(name, weights):
    csr = tg.WEIGHT_MODES[weights](ref.ring_of_cliques(6, 4))
    parts = np.array(EMPTY_PARTS[name], dtype=np.int64)
    world, nv = len(parts) - 1, int(parts[-1])
    oracle = tg.oracle_run(csr, world, parts, trace_cap=TRACE_CAP)
    _, oiters, ott, _ = oracle
    out, = run_csrs(tg.split(csr, parts), parts, TRACE_CAP, join_s=JOIN_S)
    assert sorted(out[r]["lnv"] for r in out) == sorted(np.diff(parts))
    check_vs_oracle(out, oracle, parts)
    comm = np.concatenate([out[r]["communities"] for r in range(world)])
    assert np.array_equal(comm, ref.phase_assignment(ott, oiters, nv))


# ---- G2: aggregation alone ----

COARSEN_CASES = ["nv1", "nv2", "nv65", "nv257", "no_edges", "one_community",
                 "identity_parallel", "sparse_unordered",
                 "isolated_and_loops", "community_of_1000", "parallel_5000",
                 "random_3000"]


def _parts_kinds(nv, world):
    """even always; random cuts (every rank at least one vertex) where nv
    allows them."""
    return ("even", "random") if nv - 1 >= world - 1 and world > 1 \
        else ("even",)


def _coarsen_dist(world, jobs):
    """jobs = [(csr, parts, comm)] on one set of engines -> per job
    (stitched coarse csr, stitched map, every rank's coarse parts)."""
    def body(r, e):
        res = []
        for csr, parts, comm in jobs:
            g = _slice(csr, parts, r)
            cg, cmap = e.coarsen_dist(g, comm[parts[r]:parts[r + 1]])
            res.append((cg.arrays(), cmap, cg.parts, cg.nv, cg.lnv))
            cg.free()
            g.free()
        return res

    out = _run_ranks(world, body)
    results = []
    for j in range(len(jobs)):
        per = [out[r][j] for r in range(world)]
        nc = per[0][3]
        want = tg.even_parts(nc, world)
        for r in range(world):
            assert per[r][3] == nc
            assert np.array_equal(per[r][2], want), f"rank {r}"
            assert per[r][4] == want[r + 1] - want[r]
        results.append((_stitch([p[0] for p in per]),
                        np.concatenate([p[1] for p in per])))
    return results


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("name", COARSEN_CASES)
def test_coarsen_dist_matches_numpy(name, world):
    nv, u, v, comm = _coarsen_case(name)
    comm = np.asarray(comm, dtype=np.int64)
    jobs = []
    for kind in _parts_kinds(nv, world):
        parts = dref.parts_of(kind, nv, world)
        for mode in ("unit", "int", "real"):
            fine = ref.csr_from_edges(nv, u, v, _weights(mode, len(u), 5))
            jobs.append((fine, parts, comm))
    for (fine, _, _), (got, gmap) in zip(jobs, _coarsen_dist(world, jobs)):
        assert gmap.shape == (nv,)
        _assert_coarse_equal(got, fine, comm, gmap)


@pytest.mark.parametrize("name", ["random_3000", "parallel_5000",
                                  "community_of_1000"])
def test_coarsen_dist_is_deterministic(name):
    nv, u, v, comm = _coarsen_case(name)
    comm = np.asarray(comm, dtype=np.int64)
    fine = ref.csr_from_edges(nv, u, v, _weights("real", len(u), 9))
    for world in (2, 3):
        parts = tg.even_parts(nv, world)
        a, b = _coarsen_dist(world, [(fine, parts, comm)] * 2)
        for x, y in zip(a[0] + (a[1],), b[0] + (b[1],)):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("bad", [-1, 6])
@pytest.mark.parametrize("world,where", [(2, 0), (2, 1), (3, 1)])
def test_coarsen_dist_bad_label_raises_on_every_rank(world, where, bad):
    csr = ref.clique(6)
    parts = tg.even_parts(6, world)
    comm = np.arange(6, dtype=np.int64)
    comm[parts[where]] = bad  # one label of one rank

    def body(r, e):
        g = _slice(csr, parts, r)
        try:
            e.coarsen_dist(g, comm[parts[r]:parts[r + 1]])
        except RuntimeError:
            return "raised"
        finally:
            g.free()
        return "returned"

    out = _run_ranks(world, body)
    assert out == {r: "raised" for r in range(world)}


# ---- G3: the driver, chained parity ----

MP_CASES = [("ring30", 2, "even"), ("ring30", 3, "random"),
            ("ring64", 4, "even"), ("clique5", 2, "even"),
            ("clique5", 4, "even"), ("planted", 3, "random"),
            ("adv3", 2, "even"), ("adv4", 4, "random"),
            ("rgg_unit", 2, "even"), ("rgg_unit", 4, "even"),
            ("rgg_w", 2, "even")]


def _run_dist(csr, parts, nruns=1, then=None):
    """nruns run_multiphase_dist calls on one set of engines -> per run
    {rank: snapshot}; then(rank, engine) runs afterwards on each rank."""
    world = len(parts) - 1

    def body(r, e):
        g = _slice(csr, parts, r)
        snaps = []
        for _ in range(nruns):
            h = e.run_multiphase_dist(g, thresh=THRESH)
            snaps.append(_snapshot(h, dist=True))
            h.free()
        extra = then(r, e) if then else None
        g.free()
        return snaps, extra

    out = _run_ranks(world, body)
    runs = [{r: out[r][0][k] for r in range(world)} for k in range(nruns)]
    return runs, {r: out[r][1] for r in range(world)}


@functools.lru_cache(maxsize=None)
def _mp_gpu(name, world, kind):
    csr = dref.mp_input(name)
    parts = dref.parts_of(kind, len(csr[0]) - 1, world)
    return parts, _run_dist(csr, parts)[0][0]


def _global_view(snaps, parts0):
    """Every rank reports the same global facts; -> rank 0's snapshot with
    graphs / maps / communities stitched and parts per level."""
    world = len(snaps)
    s0 = snaps[0]
    for r in range(1, world):
        s = snaps[r]
        assert (s["phases"], s["levels"]) == (s0["phases"], s0["levels"])
        assert [float(x).hex() for x in s["q"]] == \
            [float(x).hex() for x in s0["q"]], f"rank {r}"
        assert _snap_equal(s["info"], s0["info"]), f"rank {r}"
        assert _snap_equal(s["parts"], s0["parts"]), f"rank {r}"
        assert s["nv"] == s0["nv"]
    L = s0["levels"]
    parts = [np.asarray(parts0)] + s0["parts"][1:]
    for k in range(1, L + 1):
        assert np.array_equal(parts[k], tg.even_parts(s0["nv"][k], world))
    graphs = [None] + [_stitch([snaps[r]["graphs"][k] for r in range(world)])
                       for k in range(1, L + 1)]
    for k in range(1, L + 1):
        assert len(graphs[k][0]) - 1 == s0["nv"][k]
        for r in range(world):
            assert len(snaps[r]["graphs"][k][0]) - 1 == \
                parts[k][r + 1] - parts[k][r]
            assert len(snaps[r]["maps"][k]) == \
                parts[k - 1][r + 1] - parts[k - 1][r]
    maps = [None] + [np.concatenate([snaps[r]["maps"][k]
                                     for r in range(world)])
                     for k in range(1, L + 1)]
    comm = np.concatenate([snaps[r]["communities"] for r in range(world)])
    return dict(phases=s0["phases"], levels=L, graphs=graphs, parts=parts,
                maps=maps, q=s0["q"], info=s0["info"], communities=comm)


@pytest.mark.parametrize("name,world,kind", MP_CASES)
def test_multiphase_dist_chained_parity(name, world, kind):
    csr0 = dref.mp_input(name)
    parts0, snaps = _mp_gpu(name, world, kind)
    s = _global_view(snaps, parts0)
    graphs = [csr0] + s["graphs"][1:]
    P, L = s["phases"], s["levels"]
    assert 1 <= P and L <= P
    assert abs(s["q"][0] - ref.level_modularity(*csr0)) < 1e-9
    for p in range(1, P + 1):
        info = s["info"][p]
        fine = graphs[p - 1]  # every phase before the last kept its level
        nv_in = len(fine[0]) - 1
        assert (info["nv_in"], info["ne_in"]) == (nv_in, len(fine[1]))
        omod, oiters, assign = dref.oracle_phase(fine, s["parts"][p - 1],
                                                 THRESH)
        assert info["iters"] == oiters, f"phase {p}"
        assert abs(info["run_mod"] - omod) < 1e-9, f"phase {p}"
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
        assert np.array_equal(s["maps"][p], omap), f"phase {p}"
        _assert_coarse_equal(graphs[p], fine, s["maps"][p])
        assert abs(s["q"][p] - ref.level_modularity(*graphs[p])) < 1e-9
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
    sizes, iters, q, _ = dref.TABLE[name]
    assert [len(g[0]) - 1 for g in graphs[1:]] == sizes
    assert [s["info"][p]["iters"] for p in range(1, P + 1)] == iters
    assert abs(s["q"][L] - q) < 1e-9


# ---- G4: degenerate and hygiene ----

@pytest.mark.parametrize("name", ["rgg_unit", "rgg_w", "adv4"])
def test_single_rank_dist_equals_run_multiphase(name):
    from minivite_amd import Engine, Graph
    csr = dref.mp_input(name)
    nv = len(csr[0]) - 1
    g = Graph.from_csr(nv, 0, 1, np.array([0, nv], dtype=np.int64), *csr)
    e = Engine(device=0)
    snaps = []
    for run in (e.run_multiphase, e.run_multiphase_dist):
        h = run(g, thresh=THRESH)
        snaps.append(_snapshot(h, dist=True))
        h.free()
    e.destroy()
    g.free()
    assert _snap_equal(*snaps)
    assert dref.summary(dict(
        graphs=snaps[1]["graphs"],
        phases=snaps[1]["info"][1:])) == dref.TABLE[name][:2]


def test_engine_reuse_after_multiphase_dist():
    """Two distributed runs on the same engines agree bit for bit, and a
    reload + plain run afterwards reproduces the two-rank phase-one pin."""
    from minivite_amd import Graph
    pin = json.load(open(GOLDEN))["rgg_n16384_p2_unit"]
    csr = dref.mp_input("rgg_unit")
    parts = tg.even_parts(16384, 2)

    def then(r, e):
        g = Graph.rgg(16384, r, 2)
        rec, = traced_run(e, g, TRACE_CAP)
        g.free()
        return rec

    (a, b), after = _run_dist(csr, parts, nruns=2, then=then)
    for r in range(2):
        assert _snap_equal(a[r], b[r]), f"rank {r}"
        assert _snap_equal(a[r], _mp_gpu("rgg_unit", 2, "even")[1][r])
    check_vs_pin(after, pin)


# ---- G5: real RCCL, two devices ----

def _rccl_rank(rank, world, cid, q):
    try:
        from minivite_amd import Engine
        # the slices of G3: the ONE-rank RGG split evenly. Graph.rgg(nv,
        # rank, world) would be another graph (the generator's edge set
        # depends on the rank count) with another hierarchy.
        g = _slice(dref.mp_input("rgg_unit"), tg.even_parts(16384, world),
                   rank)
        e = Engine(device=rank, rank=rank, nranks=world, comm_id_bytes=cid)
        h = e.run_multiphase_dist(g, thresh=THRESH)
        L = h.levels
        q.put((rank, [h.graph(k).nv for k in range(1, L + 1)],
               [h.phase_info(p)["iters"] for p in range(1, h.phases + 1)],
               h.modularity(L)))
        h.free()
        e.destroy()
        g.free()
    except Exception as ex:  # pragma: no cover
        q.put((rank, "error", repr(ex), 0.0))


def test_multiphase_dist_rccl_p2():
    """The RCCL arm of the new exchanges -- needs two devices; skips on a
    one-GPU box."""
    import torch
    world = 2
    if torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs")
    import torch.multiprocessing as mp
    from minivite_amd import comm_id
    cid = comm_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rccl_rank, args=(r, world, cid, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        r = q.get(timeout=300)
        assert r[1] != "error", f"rank {r[0]}: {r[2]}"
        results[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
    sizes, iters, qfin, _ = dref.TABLE["rgg_unit"]
    for r in range(world):
        assert results[r][0] == sizes and results[r][1] == iters
        assert abs(results[r][2] - qfin) < 1e-9
