"""The multi-rank halo on tiny and lopsided partitions, and every arm of
its exchange plan.

The inputs (_halo_model.py, pinned on the CPU by test_halo_model_ref.py)
put one vertex on a rank, SELL-64 chunk edges (lnv 1 | 63 | 64 | 65), a
rank without edges, ranks that are all exports, and a pair of ranks where
only one side wants anything through the p>1 engine (loopback on one
device, one thread per rank). Weights are small integers, so every check
is exact. Every case demands, on every rank: the oracle's iteration count,
every target row, every modularity bit, the stitched communities(), and
Engine.halo_info() equal, field by field, to the host model of the
exchange plan -- so a wrong full/compact comparison, an arm that never
runs or a wrong candidate set fails even where the labels still come out
right.
"""
import numpy as np
import pytest

import _halo_model as hm
import _tie_graphs as tg
from _gpu_run import check_vs_oracle, knobs, run_csrs
from _multiphase_ref import phase_assignment

pytestmark = pytest.mark.gpu

TRACE_CAP = 64
WEIGHTS = ("unit", "ints123")
MODES = {"default": None, "no_overlap": "MV_NO_OVERLAP",
         "no_delta": "MV_NO_DELTA"}
_CACHE = {}


def _input(name, weights):
    """(csr, parts, oracle run on that partition); built once, read-only."""
    key = (name, weights)
    if key not in _CACHE:
        if name in hm.D1:
            gen, parts = hm.D1[name]
            base, parts = gen(), np.asarray(parts, dtype=np.int64)
        else:
            base, parts = hm.d2_input(name)
        csr = tg.WEIGHT_MODES[weights](base)
        _CACHE[key] = (csr, parts, tg.oracle_run(csr, len(parts) - 1, parts,
                                                 trace_cap=TRACE_CAP))
    return _CACHE[key]


# ---- running ----

def _run_mode(csr, parts, mode, nruns=1):
    """One loopback engine per rank on device 0, `nruns` run() calls on the
    same engines -> [{rank: record} per run]."""
    env = {MODES[mode]: "1"} if MODES[mode] else {}
    with knobs(**env):
        return run_csrs(tg.split(csr, parts), parts, TRACE_CAP, nruns,
                        join_s=120)


def _check(csr, parts, oracle, results, delta):
    """Everything a case asserts on every rank; -> the oracle's K."""
    world = len(parts) - 1
    nv = int(parts[-1])
    _, oiters, ott, _ = oracle
    check_vs_oracle(results, oracle, parts, degrees=tg.degrees(csr))
    comm = np.concatenate([results[r]["communities"] for r in range(world)])
    assert np.array_equal(comm, phase_assignment(ott, oiters, nv))
    models = {ov: hm.halo_model(csr, parts, ott, bool(ov), delta)[0]
              for ov in (0, 1)}
    for r in range(world):
        want = models[results[r]["sweep"]["overlap"]][r]
        got = results[r]["halo"]
        diff = {k: (got[k], want[k]) for k in hm.FIELDS if got[k] != want[k]}
        assert not diff, f"rank {r} halo_info (engine, model): {diff}"
        assert set(got) == set(hm.FIELDS)
    return oiters


# ---- D1: tiny and lopsided partitions ----

def _facts_one_per_rank(results, iters):
    for r, res in results.items():
        s = res["sweep"]
        assert s["ssz"] > 0 and s["nghost"] > 0, (r, s)
        if s["overlap"]:
            assert s["nexp"] == 1, (r, s)  # == lnv: the interior is empty


def _facts_clique(results, iters):
    assert iters == 2
    for r, res in results.items():
        s = res["sweep"]
        if s["overlap"]:
            assert s["nexp"] == len(res["communities"]), (r, s)


def _facts_isolated_tail(results, iters):
    s, h = results[2]["sweep"], results[2]["halo"]
    assert results[2]["lne"] == 0
    assert s["nghost"] == 0 and s["ssz"] == 0, s
    assert h["nrc_zero"] == h["prep_calls"] > 0, h
    assert h["nreq_sum"] == 0, h
    for r in (0, 1):
        assert results[r]["sweep"]["nghost"] > 0
        assert results[r]["sweep"]["ssz"] > 0


def _facts_one_way(results, iters):
    s0, s1 = results[0]["sweep"], results[1]["sweep"]
    assert s0["nghost"] > 0 and s0["ssz"] == 0, s0
    assert s1["nghost"] == 0 and s1["ssz"] > 0, s1
    assert s0["overlap"] == 0 and s1["overlap"] == 0
    h0, h1 = results[0]["halo"], results[1]["halo"]
    assert h0["send_full"] + h0["send_compact"] + h0["send_silent"] == 0
    assert h1["recv_full"] + h1["recv_compact"] + h1["recv_silent"] == 0


FACTS = {"one_per_rank": _facts_one_per_rank,
         "clique5_p5": _facts_clique, "clique5_p2": _facts_clique,
         "isolated_tail": _facts_isolated_tail, "one_way": _facts_one_way}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("name", list(hm.D1))
def test_tiny_partitions(name, weights, mode):
    csr, parts, oracle = _input(name, weights)
    results, = _run_mode(csr, parts, mode)
    iters = _check(csr, parts, oracle, results, delta=mode != "no_delta")
    overlap = {res["sweep"]["overlap"] for res in results.values()}
    assert len(overlap) == 1, "the overlap decision must be collective"
    if mode == "no_overlap":
        assert overlap == {0}
    if name.startswith("clique") and weights == "unit":
        for res in results.values():
            assert np.all(res["communities"] == 0)
    if name in FACTS:
        FACTS[name](results, iters)


# ---- D2: every arm of the plan ----

@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("name", list(hm.D2))
def test_every_arm(name, weights):
    """The model equality inside _check asserts the arm totals; the inputs
    sit on the equality edge of the rule at least once, so `>` for `>=`
    turns a full segment into a compact one and miscounts both."""
    csr, parts, oracle = _input(name, weights)
    results, = _run_mode(csr, parts, "default")
    _check(csr, parts, oracle, results, delta=True)
    halo = [res["halo"] for res in results.values()]
    send, recv = hm.arm_totals(halo)
    assert send == recv
    assert min(send.values()) > 0, send  # all three arms ran, with entries


def test_rerun_resets_last_sent():
    """Two run() calls on the same engines: the second starts from "all
    changed" again, so targets, modularity bits and the plan repeat."""
    csr, parts, oracle = _input("arms_p3", "ints123")
    first, second = _run_mode(csr, parts, "default", nruns=2)
    _check(csr, parts, oracle, first, delta=True)
    _check(csr, parts, oracle, second, delta=True)
    for r in first:
        assert second[r]["halo"] == first[r]["halo"], f"rank {r}"
        assert second[r]["mods"] == first[r]["mods"], f"rank {r}"
        assert np.array_equal(second[r]["targets"], first[r]["targets"])
        assert float(second[r]["mod"]).hex() == float(first[r]["mod"]).hex()
