"""The row chain of the lane-per-vertex sweeps, on the GPU.

k4_sweep and k4_sweep_iter1 order a row's loads by when their values are
needed: an identity-perm variant that never reads the permutation, chunk_off
and the vertex's degree and community in one trip, the community record
under the edge loop, the vertex weight from the degree (unit) or loaded once
(weighted), the gain scan as an LDS loop followed by a spill loop, and the
queue's ticket requested inside the unit's last row. None of that changes a
value. Every case here is compared with the oracle (iterations, modularity
bits, the targets of every iteration) or with the reference-pinned n=16384
results, on inputs chosen for the branches of that code
(_chain_graphs.py, pinned on the CPU by test_sweep_chain_inputs_ref.py).
"""
import pytest

import _chain_graphs as cg
import _tie_graphs as tg
from _gpu_run import (check_rgg_pin, check_vs_oracle, in_child, knobs,
                      run_ranks, run_rgg, traced_run)
from _sweep_cases import (DEFAULT_UNIT_2M, check_queue, queue_knobs,
                          untraced_runs)

pytestmark = pytest.mark.gpu


def _engine_vs_oracle(rem, mode, hint=False):
    """One engine run of the hand-built graph against the oracle; returns
    (sweep_info, iterations, nv). Graph.from_csr derives a locality hint of
    its own unless MV_NO_BFS_HINT is set while it runs; without a hint the
    engine sorts the positions by descending degree."""
    from minivite_amd import Graph
    xadj, tails, w = csr = tg.WEIGHT_MODES[mode](cg.chain_graph(rem))
    nv = len(xadj) - 1
    parts = tg.even_parts(nv, 1)

    def body(r, e):
        with knobs(MV_NO_BFS_HINT=None if hint else "1"):
            g = Graph.from_csr(nv, 0, 1, parts, xadj, tails,
                               None if mode == "unit" else w)
        rec, = traced_run(e, g, 64)
        g.free()
        return rec

    records = run_ranks(1, body)
    iters = check_vs_oracle(records, tg.oracle_run(csr), parts)
    si = records[0]["sweep"]
    assert si["unit_weights"] == (mode == "unit")
    assert si["skewed"] == 0 and si["perm_identity"] == int(hint)
    assert si["iter1_label_order"] + si["iter1_internal_order"] == 1
    assert si["general"] == iters - 1
    return si, iters, nv


@pytest.mark.parametrize("hint", [False, True])
@pytest.mark.parametrize("mode", ["unit", "ints123"])
@pytest.mark.parametrize("rem", [0, 1])
def test_hand_built_graph_matches_the_oracle(rem, mode, hint):
    """No locality hint: the degree-sorted permutation, a zero-width slice
    at the end of the image, a partial last row at nv = 1 mod 64. With the
    derived hint: the same rows through the identity variants."""
    si, _, _ = _engine_vs_oracle(rem, mode, hint)
    assert si["sched_unit"] == 0  # too few rows for the derived queue


@pytest.mark.parametrize("mode", ["unit", "ints123"])
@pytest.mark.parametrize("rem", [0, 1])
def test_hand_built_graph_on_one_block_with_the_queue(rem, mode):
    """MV_SWEEP_UNIT=3 MV_SWEEP_GRID=1 MV_SWEEP_QUEUE_FROM=1: the four
    waves of one block share 64 or 65 rows in 22 units of three (the last
    one short). Four units are the waves' ticket-free first ones; the other
    18 are handed out by ticket, requested inside the last row of the unit
    before, so a wrong ticket, base or head would run a row twice or not at
    all and the targets would differ from the oracle's. Over the
    degree-sorted order (no hint), with the partial last row at rem 1."""
    with queue_knobs(3, 1, queue_from=1):
        si, iters, nv = _engine_vs_oracle(rem, mode)
    check_queue(si, 3)
    assert si["sched_grid"] == 1
    waves = 4
    units = ((nv + 63) // 64 + 2) // 3
    assert units - waves >= 4 * waves  # several queued units per wave
    # per launch: a ticket per queued unit and a dry one per wave
    assert si["sched_tickets"] == (iters - 1) * units


def test_rgg_pin_runs_the_identity_variants():
    with queue_knobs(None, None):
        records = run_rgg(16384, 1)
    check_rgg_pin(records, 1)
    assert records[0]["sweep"]["perm_identity"] == 1


def test_rgg_2m_identity_variant_under_the_shipped_schedule():
    res, si = untraced_runs(1 << 21, 2)
    assert si["perm_identity"] == 1
    check_queue(si, DEFAULT_UNIT_2M)
    assert res[0] == res[1]


def test_loopback_exports_first_order_is_not_the_identity():
    with queue_knobs(None, None):
        records = run_rgg(16384, 2)
    check_rgg_pin(records, 2)
    for r in range(2):
        si = records[r]["sweep"]
        # both ranks of this split export vertices and the loopback
        # transport always has a second channel, so the overlap and with it
        # the exports-first order are on: the check below is never vacuous
        assert si["overlap"] == 1 and si["nexp"] > 0, f"rank {r}"
        if si["overlap"] == 1:
            assert si["perm_identity"] == 0, f"rank {r}"


@pytest.mark.parametrize("unit", [True, False])
def test_spill_loop_after_the_scan_split(unit):
    """Four slots in every k4_sweep launch (iteration 2 on): most lanes of
    the first launches overflow into the spill, which the gain scan now
    reads in a loop of its own. The knobs are read once per process."""
    records = in_child(f"rgg:16384:{'unit' if unit else 'w'}", 1,
                       {"MV_SLOTS": "4", "MV_SLOTS_FIRST": "4"})
    check_rgg_pin(records, 1, unit)
