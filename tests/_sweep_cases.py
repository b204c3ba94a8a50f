"""Inputs and checks that several GPU sweep tests share: the oracle-parity
case with its routing expectations (test_gpu_tie_parity, test_gpu_unit_counts,
test_gpu_sweep_queue), the row-queue accounting and the tiny chordal ring
(test_gpu_degree_windows, test_gpu_sweep_queue, test_gpu_sweep_chain)."""
import numpy as np

import _tie_graphs as tg
from _gpu_run import TRACE_CAP, check_vs_oracle, knobs, run_csrs, run_ranks

DEFAULT_UNIT_2M = 2  # choose_row_queue's rule at n=2^21 (4 rows per wave)


def tiny_csr(lnv):
    """A chordal ring over the vertices that are not isolated (every 7th
    is), with a self-loop on vertex 0. Rows ascending, symmetric."""
    live = [v for v in range(lnv) if v % 7 != 3]
    pairs = {(0, 0)}
    for k, v in enumerate(live):
        for step in (1, 3):
            u = live[(k + step) % len(live)]
            if u != v:
                pairs.add((v, u))
                pairs.add((u, v))
    pairs = sorted(pairs)
    xadj = np.zeros(lnv + 1, dtype=np.int64)
    for v, _ in pairs:
        xadj[v + 1] += 1
    return np.cumsum(xadj), np.array([u for _, u in pairs], dtype=np.int64)


def queue_knobs(unit, grid, window=None, queue_from=None):
    """The four knobs of the sweep schedule, each set or (None) unset."""
    return knobs(MV_SWEEP_UNIT=unit, MV_SWEEP_GRID=grid,
                 MV_DEG_WINDOW=window, MV_SWEEP_QUEUE_FROM=queue_from)


def untraced_runs(nv, runs):
    """With no schedule knob set, load the RGG and run() it `runs` times
    without a trace -> ([(modularity bits, iterations, hash of
    communities()) per run], sweep_info after the last)."""
    from minivite_amd import Graph
    from oracle.oracle import sha

    def body(r, e):
        g = Graph.rgg(nv)
        e.load_graph(g)
        res = []
        for _ in range(runs):
            mod, iters = e.run()
            res.append((float(mod).hex(), iters, sha(e.communities())))
        si = e.sweep_info()
        g.free()
        return res, si

    with queue_knobs(None, None):
        return run_ranks(1, body)[0]


def check_queue(si, unit, where=""):
    assert si["sched_unit"] == unit, f"{where}{si}"
    assert si["sched_tickets"] == si["sched_tickets_expected"], f"{where}{si}"
    if unit:
        assert si["sched_tickets"] > 0, f"{where}{si}"
    else:
        assert si["sched_tickets"] == 0, f"{where}{si}"


def run_parity(csr, parts):
    """One engine per rank on the split of `csr`; iteration count, every
    target row and every modularity bit, on every rank, against the oracle
    on the same partition. -> ({rank: record}, iterations)"""
    records, = run_csrs(tg.split(csr, parts), parts, TRACE_CAP, join_s=300)
    return records, check_parity(csr, parts, records)


def check_parity(csr, parts, records):
    oracle = tg.oracle_run(csr, len(parts) - 1, parts, trace_cap=TRACE_CAP)
    return check_vs_oracle(records, oracle, parts, degrees=tg.degrees(csr))


def check_routing(info, iters, expect, where=""):
    """expect: {sweep_info key or ('slots', S): value}; a value is an int,
    '>0', or 'iters' / 'iters-N' (relative to the run's iteration count)."""
    for key, want in expect.items():
        got = info["general_slots"][key[1]] if isinstance(key, tuple) \
            else info[key]
        if want == ">0":
            assert got > 0, f"{where}{key}: {got}, expected > 0 -- {info}"
            continue
        if isinstance(want, str):
            want = iters - int(want[len("iters-"):] or 0)
        assert got == want, f"{where}{key}: {got}, expected {want} -- {info}"


def parity_case(csr, expect, parts=None, rank_expect=None):
    """Run, compare with the oracle, then check the routing: `expect` on
    every rank, rank_expect[r] on rank r. -> {rank: record}"""
    nv = len(csr[0]) - 1
    parts = tg.even_parts(nv, 1) if parts is None else \
        np.asarray(parts, dtype=np.int64)
    records, iters = run_parity(csr, parts)
    for r in sorted(records):
        check_routing(records[r]["sweep"], iters, expect, f"rank {r} ")
        if rank_expect:
            check_routing(records[r]["sweep"], iters, rank_expect[r],
                          f"rank {r} ")
    return records
