"""CPU checks for the multi-phase feature: the host reference driver
(tests/_multiphase_ref.py: numpy aggregation + the oracle once per phase)
is pinned to hand-checkable graphs, and the Python surface exists. The GPU
suite (test_gpu_multiphase.py) compares the engine against this reference,
so these constants pin the yardstick itself."""
import numpy as np

import _multiphase_ref as ref


def _summary(h):
    return ([len(g[0]) - 1 for g in h["graphs"][1:]],
            [p["iters"] for p in h["phases"]])


def test_ring_of_30_five_cliques():
    g = ref.ring_of_cliques(30, 5)
    h = ref.run_multiphase(*g)
    sizes, iters = _summary(h)
    assert sizes == [30] and iters == [4, 3]
    assert h["q"][1] == 0.8757575757575757
    p2 = h["phases"][1]  # proposes 28 communities at a lower q: dropped
    assert (p2["nv_out"], p2["kept"]) == (28, False)
    assert abs(p2["q_out"] - 0.875152) < 5e-7
    assert np.array_equal(h["communities"], np.arange(150) // 5)


def test_ring_of_64_six_cliques():
    h = ref.run_multiphase(*ref.ring_of_cliques(64, 6))
    sizes, iters = _summary(h)
    assert sizes == [64, 62, 32] and iters == [4, 3, 32, 2]
    assert h["q"][-1] == 0.93701171875
    assert all(b >= a for a, b in zip(h["q"], h["q"][1:]))


def test_single_clique_takes_the_k2_branch():
    h = ref.run_multiphase(*ref.clique(5))
    sizes, iters = _summary(h)
    assert sizes == [1] and iters[0] == 2  # merged in 1, exit in 2
    assert h["q"][1] == 0.0
    assert len(h["phases"]) == 2 and not h["phases"][1]["kept"]
    assert np.array_equal(h["communities"], np.zeros(5, dtype=np.int64))


def test_final_q_is_the_modularity_on_the_original_graph():
    g = ref.planted()
    h = ref.run_multiphase(*g)
    q = ref.partition_modularity(*g, h["communities"])
    assert abs(q - h["q"][-1]) < 1e-12
    assert h["communities"].max() + 1 == len(h["graphs"][-1][0]) - 1


def test_coarsen_definition_on_a_hand_example():
    # triangle 0-1-2 (unit) + self-loop on 2 (w=3) + pendant 3-2 (w=2);
    # communities {0,1} -> label 1, {2,3} -> label 3
    u = [0, 1, 0, 2, 1, 2, 2, 2, 3]
    v = [1, 0, 2, 0, 2, 1, 2, 3, 2]
    w = [1, 1, 1, 1, 1, 1, 3, 2, 2]
    xadj, tails, wts = ref.csr_from_edges(4, u, v, np.array(w, float))
    cx, ct, cw, cmap, runs = ref.coarsen(xadj, tails, wts, [1, 1, 3, 3])
    assert cmap.tolist() == [0, 0, 1, 1]
    assert cx.tolist() == [0, 2, 4] and ct.tolist() == [0, 1, 0, 1]
    # intra edge 0-1 stored twice -> 2; cut 2; {2,3}: loop 3 + 2*2
    assert cw.tolist() == [2.0, 2.0, 2.0, 7.0]
    assert runs.tolist() == [2, 2, 2, 3]
    assert cw.sum() == wts.sum()


def test_python_surface():
    import minivite_amd
    from minivite_amd import Engine, Hierarchy, coarsen_csr
    assert callable(Engine.run_multiphase) and callable(Engine.communities)
    assert callable(coarsen_csr)
    for name in ("phases", "levels", "graph", "map", "modularity",
                 "phase_info", "communities", "free"):
        assert hasattr(Hierarchy, name), name
    L = minivite_amd.lib()
    for sym in ("mv_engine_get_communities", "mv_coarsen_csr",
                "mv_engine_run_multiphase", "mv_hierarchy_free"):
        assert hasattr(L, sym), sym
