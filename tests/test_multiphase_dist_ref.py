"""CPU pins for the multi-phase driver across ranks. The host model
(tests/_multiphase_dist_ref.py: the oracle once per phase on that level's
partition, numpy aggregation of the stitched level, an even split for the
next level) must reproduce the single-rank reference's hierarchy at every
rank count and partition: level sizes, iterations per phase and the final
q. The GPU suite (test_gpu_multiphase_dist.py) compares the engines against
this model, so these constants pin the yardstick itself."""
import functools

import numpy as np
import pytest

import _multiphase_dist_ref as dref
import _multiphase_ref as ref
import _tie_graphs as tg


@functools.lru_cache(maxsize=None)
def _single(name):
    return ref.run_multiphase(*dref.mp_input(name))


def _cases():
    for name in dref.TABLE:
        rgg = name.startswith("rgg")
        for world in ((1, 2, 4) if rgg else (1, 2, 3, 4)):
            for kind in (("even",) if rgg or world == 1
                         else ("even", "random")):
                yield name, world, kind


@pytest.mark.parametrize("name", list(dref.TABLE))
def test_single_rank_reference_matches_the_table(name):
    sizes, iters, q, exact = dref.TABLE[name]
    h = _single(name)
    assert dref.summary(h) == (sizes, iters)
    if exact:
        assert h["q"][-1] == q
    else:
        assert abs(h["q"][-1] - q) < 1e-9


@pytest.mark.parametrize("name,world,kind", list(_cases()))
def test_hierarchy_is_independent_of_the_partition(name, world, kind):
    sizes, iters, q, exact = dref.TABLE[name]
    csr = dref.mp_input(name)
    nv = len(csr[0]) - 1
    h = dref.run_multiphase_dist(csr, dref.parts_of(kind, nv, world))
    one = _single(name)
    assert dref.summary(h) == dref.summary(one) == (sizes, iters)
    assert len(h["phases"]) == len(one["phases"])
    if exact:
        assert h["q"][-1] == one["q"][-1] == q
    else:
        assert abs(h["q"][-1] - one["q"][-1]) < 1e-9
        assert abs(h["q"][-1] - q) < 1e-9
    for a, b in zip(h["phases"], one["phases"]):
        assert (a["nv_in"], a["nv_out"], a["kept"]) == \
            (b["nv_in"], b["nv_out"], b["kept"])
    for k in range(1, len(h["graphs"])):
        assert np.array_equal(h["parts"][k], tg.even_parts(sizes[k - 1],
                                                           world))
    assert np.array_equal(h["communities"], one["communities"])


def test_levels_smaller_than_the_rank_count_leave_ranks_empty():
    h = dref.run_multiphase_dist(dref.mp_input("clique5"),
                                 tg.even_parts(5, 4))
    assert h["parts"][1].tolist() == [0, 0, 0, 0, 1]
    assert [p["iters"] for p in h["phases"]] == [2, 2]


@pytest.mark.parametrize("parts", [[0, 24, 24], [0, 0, 24], [0, 3, 3, 24]])
def test_oracle_accepts_ranks_without_vertices(parts):
    csr = ref.ring_of_cliques(6, 4)
    parts = np.array(parts, dtype=np.int64)
    mod, iters, _, _ = tg.oracle_run(csr, len(parts) - 1, parts)
    one = tg.oracle_run(csr)
    assert (mod, iters) == (0.6904761904761905, 4)
    assert (one[0], one[1]) == (mod, iters)


@pytest.mark.parametrize("mode", ["unit", "int", "real"])
def test_two_stage_weight_sum(mode):
    """Per-rank partials added in rank order: exact for integer-valued
    weights, else within (m-1) * 2^-52 * w of numpy's one-stage sum, m =
    fine edges of the run (any order of m positive doubles is)."""
    rng = np.random.default_rng(3)
    nv, m = 300, 6000
    u, v = rng.integers(0, nv, m), rng.integers(0, nv, m)
    w = {"unit": np.ones(m), "int": rng.integers(1, 9, m).astype(float),
         "real": rng.uniform(0.01, 1.0, m)}[mode]
    csr = ref.csr_from_edges(nv, u, v, w)
    comm = rng.integers(0, 12, nv) * 5
    _, _, cw, _, runs = ref.coarsen(*csr, comm)
    for world in (1, 2, 3, 4):
        for kind in ("even", "random"):
            parts = dref.parts_of(kind, nv, world)
            got = dref.coarse_weights_two_stage(csr, parts, comm)
            if mode == "real":
                assert np.all(np.abs(got - cw) <= (runs - 1) * 2.0 ** -52 * cw)
            else:
                assert np.array_equal(got, cw)


def test_python_surface():
    import minivite_amd
    from minivite_amd import Engine, Graph
    assert callable(Engine.run_multiphase_dist)
    assert callable(Engine.coarsen_dist)
    assert isinstance(Graph.parts, property)
    L = minivite_amd.lib()
    for sym in ("mv_engine_coarsen_dist", "mv_engine_run_multiphase_dist",
                "mv_graph_rank", "mv_graph_nranks"):
        assert hasattr(L, sym), sym
    xadj, tails, w = ref.clique(5)
    parts = np.array([0, 0, 5], dtype=np.int64)
    g = Graph.from_csr(5, 1, 2, parts, xadj, tails, w)
    assert g.parts.tolist() == [0, 0, 5] and not g.parts.flags.writeable
    g.free()
    empty = Graph.from_csr(5, 0, 2, parts, np.zeros(1, dtype=np.int64),
                           np.zeros(0, dtype=np.int64), np.zeros(0))
    assert (empty.lnv, empty.lne) == (0, 0)
    empty.free()
