"""The one place the GPU tests start engines.

run_ranks() puts a body on one engine per rank (inline at one rank, loopback
engines on threads otherwise), traced_run() is the standard body and yields
the one result shape (a record, below), stitch() / check_vs_pin() /
check_vs_oracle() compare records, knobs() sets MV_* variables and puts the
environment back, in_child() runs _engine_child.py in a fresh process for
the tunables that are read once per process.

A record is a dict: mod, iters, targets (a copy of the trace rows), mods
(per-iteration modularity as hex strings), sweep (Engine.sweep_info()), halo
(Engine.halo_info()), communities, lnv, lne, sweep_launches.
"""
import contextlib
import json
import os
import subprocess
import sys
import tempfile
import threading
import traceback

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pins.json")
CHILD = os.path.join(HERE, "_engine_child.py")
TRACE_CAP = 64
_ARRAYS = ("targets", "communities")  # record fields a child sends as .npz
_leaked = []  # sessions of hung runs: referenced for good, never destroyed


# ---- running ----

def run_ranks(world, body, join_s=600, _mv=None):
    """body(rank, engine) on one engine per rank -> {rank: body's value}.

    One rank runs inline on Engine(device=0). Several run as loopback
    engines of one session on device 0, a daemon thread each, joined for
    `join_s` seconds each. A thread still alive after that may be inside a
    kernel or a barrier of the session: the session is then leaked, not
    destroyed, and the whole pytest session ends, so that nothing else is
    started on that GPU. Otherwise the session is destroyed and one
    assertion names every rank whose body raised."""
    if _mv is None:
        import minivite_amd as _mv
    if world == 1:
        e = _mv.Engine(device=0)
        try:
            return {0: body(0, e)}
        finally:
            e.destroy()
    ses = _mv.LoopbackSession(world)
    out, errors = {}, {}

    def rank_main(r):
        e = None
        try:
            e = _mv.Engine.loopback(ses, r, device=0)
            out[r] = body(r, e)
        except Exception:
            errors[r] = traceback.format_exc()
        finally:
            if e is not None:
                e.destroy()

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True)
               for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=join_s)
    alive = [r for r, t in enumerate(threads) if t.is_alive()]
    if alive:
        ses.destroy = lambda: None  # not by __del__ either
        _leaked.append(ses)
        pytest.exit(f"loopback rank(s) {alive} of {world} still running "
                    f"after {join_s} s; the session is leaked and nothing "
                    "more may run on this GPU", returncode=3)
    ses.destroy()
    assert not errors, "rank(s) %s raised:\n%s" % (
        sorted(errors), "\n".join(errors[r] for r in sorted(errors)))
    return out


def traced_run(engine, graph, trace_cap=TRACE_CAP, nruns=1):
    """Load `graph`, arm the trace, run() `nruns` times -> a record per
    run."""
    engine.load_graph(graph)
    engine.set_trace(trace_cap)
    records = []
    for _ in range(nruns):
        mod, iters = engine.run()
        tt, tm = engine.trace(iters)
        records.append(dict(
            mod=mod, iters=iters, targets=tt.copy(),
            mods=[float(m).hex() for m in tm], sweep=engine.sweep_info(),
            halo=engine.halo_info(), communities=engine.communities(),
            lnv=graph.lnv, lne=graph.lne,
            sweep_launches=engine.stats()["sweep_launches"]))
    return records


def by_run(out):
    """{rank: [record per run]} -> [{rank: record} per run]."""
    return [{r: out[r][k] for r in out} for k in range(len(out[0]))]


def run_rgg(nv, world, unit=True, trace_cap=TRACE_CAP, join_s=600):
    """The generated RGG, split evenly -> {rank: record}."""
    from minivite_amd import Graph

    def body(r, e):
        g = Graph.rgg(nv, r, world, unit_weight=unit)
        rec, = traced_run(e, g, trace_cap)
        g.free()
        return rec

    return run_ranks(world, body, join_s)


def run_csrs(csrs, parts, trace_cap=TRACE_CAP, nruns=1, join_s=600):
    """Per-rank (xadj, tails, w) slices of the partition `parts`, `nruns`
    run() calls on the same engines -> [{rank: record} per run]."""
    from minivite_amd import Graph
    parts = np.asarray(parts, dtype=np.int64)
    world = len(parts) - 1

    def body(r, e):
        g = Graph.from_csr(int(parts[-1]), r, world, parts, *csrs[r])
        recs = traced_run(e, g, trace_cap, nruns)
        g.free()
        return recs

    return by_run(run_ranks(world, body, join_s))


# ---- comparing ----

def stitch(records, parts):
    """Per-rank target rows -> the global (rows, nv) array."""
    full = np.zeros((len(records[0]["targets"]), int(parts[-1])),
                    dtype=np.int64)
    for r in range(len(parts) - 1):
        full[:, parts[r]:parts[r + 1]] = records[r]["targets"]
    return full


def _check_iters(records, world, iters):
    assert sorted(records) == list(range(world))
    for r in range(world):
        assert records[r]["iters"] == iters, f"rank {r}"


def _check_mods(records, mod, mods, exact_mod):
    """Every rank reports the global modularity: the same bits, in every
    iteration too, or within 1e-9."""
    for r in sorted(records):
        rec = records[r]
        if exact_mod:
            assert float(rec["mod"]).hex() == float(mod).hex(), f"rank {r}"
            assert rec["mods"] == mods, f"rank {r}"
        else:
            assert abs(rec["mod"] - mod) < 1e-9, f"rank {r}"


def check_vs_pin(records, pin, exact_mod=True):
    """{rank: record} of the evenly split RGG against its reference pin:
    iterations, final modularity (bits, or within 1e-9) and, with
    exact_mod, every iteration's modularity bits on every rank; every
    stitched target row by hash. -> iterations"""
    from oracle.oracle import sha
    world, nv = len(records), pin["nv"]
    _check_iters(records, world, pin["iters"])
    _check_mods(records, float.fromhex(pin["final_mod_hex"]),
                pin["iter_mod_hex"], exact_mod)
    full = stitch(records, [(nv * r) // world for r in range(world + 1)])
    assert len(full) == len(pin["iter_target_sha"])
    for k, row in enumerate(full):
        assert sha(row) == pin["iter_target_sha"][k], f"iteration {k + 1}"
    if world == 1:  # the pinned RGGs are not skewed: one sweep per iteration
        assert records[0]["sweep_launches"] == pin["iters"]
    return pin["iters"]


def check_rgg_pin(records, world, unit=True):
    """check_vs_pin against the n=16384 pin of that rank count and weight
    kind (weighted: modularity within 1e-9)."""
    assert len(records) == world
    pin = json.load(open(GOLDEN))[
        f"rgg_n16384_p{world}_{'unit' if unit else 'w'}"]
    return check_vs_pin(records, pin, exact_mod=unit)


def check_vs_oracle(records, oracle_result, parts, exact_mod=True,
                    degrees=None):
    """{rank: record} against (mod, iters, target rows, per-iteration
    modularity) of the oracle on the same partition: iterations and final
    modularity (bits, or within 1e-9) on every rank, with exact_mod every
    iteration's modularity bits too, and every target row.
    A target mismatch names the first differing iteration, vertex, its
    degree (given `degrees`) and rank. -> iterations"""
    omod, oiters, ott, otm = oracle_result
    parts = np.asarray(parts, dtype=np.int64)
    _check_iters(records, len(parts) - 1, oiters)
    full = stitch(records, parts)
    ott = np.asarray(ott)[:len(full)]
    bad = np.argwhere(full != ott)
    if bad.size:
        k, v = bad[0]
        deg = "?" if degrees is None else degrees[v]
        pytest.fail(
            f"{len(bad)} targets differ; first at iteration {k + 1} vertex "
            f"{v} (degree {deg}, rank "
            f"{int(np.searchsorted(parts, v, 'right')) - 1}): engine "
            f"{full[k, v]} oracle {ott[k, v]}")
    assert np.array_equal(full, ott)
    _check_mods(records, omod, [float(m).hex() for m in otm[:len(full)]],
                exact_mod)
    return oiters


# ---- the environment ----

@contextlib.contextmanager
def knobs(**env):
    """Set each variable (None: unset it) for the body; afterwards every
    one is what it was before, unset or set to some other value."""
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def in_child(spec, world, env, timeout=120):
    """_engine_child.py on the graph `spec` in a fresh process with `env`
    added -> {rank: record}, as run_ranks would have returned them."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace.npz")
        child = subprocess.run(
            [sys.executable, CHILD, spec, str(world), path],
            env=dict(os.environ, **env), capture_output=True, text=True,
            timeout=timeout)
        assert child.returncode == 0, child.stderr[-2000:]
        out = json.loads(child.stdout.strip().splitlines()[-1])
        z = np.load(path)
        records = {}
        for r in range(world):
            rec = out[str(r)]
            rec["sweep"]["general_slots"] = {
                int(k): v for k, v in rec["sweep"]["general_slots"].items()}
            rec.update((f, z[f"{f}{r}"]) for f in _ARRAYS)
            records[r] = rec
    return records
