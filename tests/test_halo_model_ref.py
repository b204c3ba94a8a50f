"""CPU yardstick for the halo inputs and the halo model (_halo_model.py).

Nothing here touches a GPU. It checks the model against two hand-worked
plans, and pins -- with the oracle alone -- that the inputs
test_gpu_halo_edges.py feeds the engines are what they are meant to be:
every D2 input makes the model report all three arms AND the equality edge
of the full/compact rule, the tiny and lopsided D1 partitions have the
shapes they are named for, and the oracle's result on each input does not
depend on the partition (integer weights make that exact).
"""
import functools

import numpy as np
import pytest

import _halo_model as hm
import _tie_graphs as tg

WEIGHTS = ("unit", "ints123")
D1_CASES = [(n, w) for n in hm.D1 for w in WEIGHTS]
D2_CASES = [(n, w) for n in hm.D2 for w in WEIGHTS]


@functools.lru_cache(maxsize=None)
def _input(name, weights):
    if name in hm.D1:
        gen, parts = hm.D1[name]
        base, parts = gen(), np.asarray(parts, dtype=np.int64)
    else:
        base, parts = hm.d2_input(name)
    return tg.WEIGHT_MODES[weights](base), parts


@functools.lru_cache(maxsize=None)
def _oracle(name, weights, partitioned=True):
    """(mod, iters, targets, mods); read-only for every test."""
    csr, parts = _input(name, weights)
    if partitioned:
        return tg.oracle_run(csr, len(parts) - 1, parts)
    return tg.oracle_run(csr, 1)


def _hex(a):
    return [float(x).hex() for x in a]


# ---- the model against plans worked out by hand ----

def test_model_path_by_hand():
    """Path 0-1-2-3 cut in the middle: one-entry segments 0->1 = [1] and
    1->0 = [2]. Wire: identity, then [0,0,2,2] twice. Exchange 1: both
    changed -> full. Exchange 2: vertex 1 went 1->0 (full, 12 >= 8),
    vertex 2 kept 2 (silent). Exchange 3: both silent. Each rank always
    sees exactly one remote label."""
    csr = hm.symmetric(4, [0, 1, 2], [1, 2, 3])
    row = np.array([0, 0, 2, 2])
    info, boundary = hm.halo_model(csr, [0, 2, 4], [row, row, row], False)
    assert boundary == 0
    common = dict(exchanges=3, send_compact=0, recv_compact=0,
                  send_compact_entries=0, recv_compact_entries=0,
                  prep_calls=3, nrc_sum=3, nrc_max=1, nrc_zero=0, nreq_sum=3)
    assert info[0] == dict(common, send_full=2, send_silent=1, recv_full=1,
                           recv_silent=2)
    assert info[1] == dict(common, send_full=1, send_silent=2, recv_full=2,
                           recv_silent=1)
    assert set(info[0]) == set(hm.FIELDS)


def test_model_star_by_hand():
    """Star: vertex 0 alone on rank 0, leaves 1..3 on rank 1. Segment
    1->0 = [1,2,3], 0->1 = [0]. Wire: identity, [0,0,0,3], [0,0,0,0] and,
    with the overlap, [0,0,0,0] again.
      1->0: 3 of 3 full; 2 of 3 -> 24 >= 24, full ON THE EDGE; 1 of 3 ->
            12 < 24, one pair; 0 of 3 silent.
      0->1: full, then silent ever after.
    Rank 0 requests {1,2,3}, then {3}, then nothing; rank 1 requests {0}
    every time (vertex 3 holds out for one exchange, then joins 0)."""
    csr = hm.symmetric(4, [0, 0, 0], [1, 2, 3])
    rows = [np.array([0, 0, 0, 3]), np.array([0, 0, 0, 0]),
            np.array([0, 0, 0, 0])]
    info, boundary = hm.halo_model(csr, [0, 1, 4], rows, False)
    assert boundary == 1
    assert info[1] == dict(
        exchanges=3, send_full=2, send_compact=1, send_silent=0,
        recv_full=1, recv_compact=0, recv_silent=2, send_compact_entries=1,
        recv_compact_entries=0, prep_calls=3, nrc_sum=3, nrc_max=1,
        nrc_zero=0, nreq_sum=4)
    assert info[0] == dict(
        exchanges=3, send_full=1, send_compact=0, send_silent=2,
        recv_full=2, recv_compact=1, recv_silent=0, send_compact_entries=0,
        recv_compact_entries=1, prep_calls=3, nrc_sum=4, nrc_max=3,
        nrc_zero=1, nreq_sum=3)
    over, boundary = hm.halo_model(csr, [0, 1, 4], rows, True)
    assert boundary == 1
    assert over[1] == dict(info[1], exchanges=4, prep_calls=4,
                           send_silent=1, recv_silent=3, nrc_sum=4,
                           nreq_sum=4)
    assert over[0] == dict(info[0], exchanges=4, prep_calls=4,
                           send_silent=3, recv_silent=1, nrc_zero=2,
                           nreq_sum=4)


def test_full_mode_edge():
    assert hm.full_mode(2, 3) and not hm.full_mode(1, 3)
    assert hm.full_mode(4, 6) and not hm.full_mode(3, 6)
    assert hm.full_mode(1, 1) and not hm.full_mode(0, 1)
    assert hm.full_mode(0, 0)  # an empty segment is never planned


# ---- D2: every arm and the equality edge, on every input ----

@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("name,weights", D2_CASES)
def test_d2_inputs_reach_every_arm(name, weights, overlap):
    csr, parts = _input(name, weights)
    assert 24 <= parts[-1] <= 96
    _, iters, tt, _ = _oracle(name, weights)
    info, boundary = hm.halo_model(csr, parts, tt, overlap)
    send, _ = hm.arm_totals(info)
    print(f"{name}/{weights} overlap={int(overlap)}: K {iters} {send} "
          f"boundary {boundary}")
    assert send["full"] > 0
    assert send["compact"] > 0 and send["compact_entries"] > 0
    assert send["silent"] > 0
    assert boundary > 0


# ---- properties of the model on every input ----

@pytest.mark.parametrize("delta", [True, False])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("name,weights", D1_CASES + D2_CASES)
def test_sends_equal_receives(name, weights, overlap, delta):
    csr, parts = _input(name, weights)
    _, iters, tt, _ = _oracle(name, weights)
    info, boundary = hm.halo_model(csr, parts, tt, overlap, delta)
    send, recv = hm.arm_totals(info)
    assert send == recv
    nseg = sum(1 for a, g in enumerate(hm.ghosts_of(csr, parts))
               for b in np.unique(np.searchsorted(parts, g, "right") - 1))
    nex = iters + int(overlap)
    assert send["full"] + send["compact"] + send["silent"] == nseg * nex
    for d in info:
        assert d["exchanges"] == d["prep_calls"] == nex
        assert d["nrc_max"] <= d["nrc_sum"]
    assert sum(d["nrc_sum"] for d in info) == \
        sum(d["nreq_sum"] for d in info)
    if not delta:
        assert boundary == 0
        assert send["compact"] == send["silent"] == 0
        assert send["compact_entries"] == 0
        assert send["full"] == nseg * nex


@pytest.mark.parametrize("name,weights", D1_CASES + D2_CASES)
def test_single_rank_is_all_zero(name, weights):
    csr, parts = _input(name, weights)
    _, _, tt, _ = _oracle(name, weights)
    for overlap in (False, True):
        info, boundary = hm.halo_model(csr, [0, parts[-1]], tt, overlap)
        assert info == [dict.fromkeys(hm.FIELDS, 0)] and boundary == 0


@pytest.mark.parametrize("name,weights", D1_CASES + D2_CASES)
def test_partition_invariance(name, weights):
    mod, iters, tt, tm = _oracle(name, weights)
    m1, i1, t1, tm1 = _oracle(name, weights, partitioned=False)
    assert 2 <= iters == i1
    assert np.array_equal(tt, t1)
    assert _hex(tm) == _hex(tm1) and float(mod).hex() == float(m1).hex()


# ---- D1: the shapes the cases are named for ----

def _rank_shapes(name):
    csr, parts = _input(name, "unit")
    lnv = np.diff(parts)
    lne = np.array([csr[0][hi] - csr[0][lo]
                    for lo, hi in zip(parts[:-1], parts[1:])])
    ghosts = hm.ghosts_of(csr, parts)
    nghost = np.array([g.size for g in ghosts])
    ssz = np.zeros(len(lnv), dtype=np.int64)
    exported = [set() for _ in lnv]
    for g in ghosts:
        owner = np.searchsorted(parts, g, "right") - 1
        np.add.at(ssz, owner, 1)
        for v, b in zip(g.tolist(), owner.tolist()):
            exported[b].add(v)
    nexp = np.array([len(s) for s in exported])
    return lnv, lne, nghost, ssz, nexp


def test_d1_shapes():
    lnv, lne, nghost, ssz, nexp = _rank_shapes("one_per_rank")
    assert np.all(lnv == 1) and len(lnv) == 8
    assert np.all(ssz > 0) and np.all(nexp == lnv)  # no interior anywhere
    assert np.all(nghost == lne)                    # every edge is remote

    lnv, lne, nghost, ssz, nexp = _rank_shapes("nine_p8")
    assert lnv.tolist() == [1] * 7 + [2] and np.all(ssz > 0)

    lnv, lne, nghost, ssz, nexp = _rank_shapes("chunk_edges")
    assert lnv.tolist() == [1, 63, 64, 65]  # around one SELL-64 chunk
    assert np.all(nghost > 0) and np.all(ssz > 0)

    for name in ("clique5_p5", "clique5_p2"):
        lnv, lne, nghost, ssz, nexp = _rank_shapes(name)
        assert np.all(nexp == lnv)  # a clique: every vertex is an export
        _, iters, tt, _ = _oracle(name, "unit")
        assert iters == 2 and np.all(tt[0] == 0)
        assert _oracle(name, "ints123")[1] == 2

    lnv, lne, nghost, ssz, nexp = _rank_shapes("isolated_tail")
    assert lnv.tolist() == [50, 50, 20]
    assert lne[2] == 0 and nghost[2] == 0 and ssz[2] == 0
    assert np.all(nghost[:2] > 0) and np.all(ssz[:2] > 0)

    lnv, lne, nghost, ssz, nexp = _rank_shapes("one_way")
    assert lnv.tolist() == [30, 30]
    assert nghost[0] > 0 and ssz[0] == 0  # rank 0 wants, is asked nothing
    assert nghost[1] == 0 and ssz[1] > 0  # rank 1 the reverse


def test_d1_has_length_one_segments():
    """Segments of length 1 exist wherever a rank holds one vertex."""
    for name in ("one_per_rank", "nine_p8", "chunk_edges", "clique5_p5"):
        csr, parts = _input(name, "unit")
        sizes = []
        for g in hm.ghosts_of(csr, parts):
            owner = np.searchsorted(parts, g, "right") - 1
            sizes += np.bincount(owner)[np.unique(owner)].tolist()
        assert 1 in sizes, name
