"""_gpu_run.py without a GPU: knobs() puts the environment back, stitch()
takes uneven and empty parts, run_ranks() collects, reports and, when a rank
hangs, leaks the session and ends the pytest session."""
import os
import threading
import types

import numpy as np
import pytest

from _gpu_run import knobs, run_ranks, stitch


def test_knobs_restore_the_environment(monkeypatch):
    monkeypatch.delenv("MV_T_UNSET", raising=False)
    monkeypatch.setenv("MV_T_SET", "before")
    monkeypatch.setenv("MV_T_DROP", "kept")
    with knobs(MV_T_UNSET=3, MV_T_SET="during", MV_T_DROP=None):
        assert os.environ["MV_T_UNSET"] == "3"
        assert os.environ["MV_T_SET"] == "during"
        assert "MV_T_DROP" not in os.environ
    with pytest.raises(KeyError):
        with knobs(MV_T_UNSET="x", MV_T_SET="y", MV_T_DROP=None):
            raise KeyError("body")
    assert "MV_T_UNSET" not in os.environ
    assert os.environ["MV_T_SET"] == "before"
    assert os.environ["MV_T_DROP"] == "kept"


def test_stitch_uneven_parts_with_an_empty_rank():
    parts = [0, 3, 3, 24]
    rows = np.arange(2 * 24).reshape(2, 24)
    records = {r: {"targets": rows[:, parts[r]:parts[r + 1]]}
               for r in range(3)}
    assert records[1]["targets"].shape == (2, 0)
    assert np.array_equal(stitch(records, parts), rows)


def _fake():
    """A stand-in for the minivite_amd module that counts its calls."""
    log = types.SimpleNamespace(engines=0, engines_destroyed=0, sessions=0,
                                sessions_destroyed=0, lock=threading.Lock())

    def count(name):
        with log.lock:
            setattr(log, name, getattr(log, name) + 1)

    class Session:
        def __init__(self, nranks):
            self.nranks = nranks
            count("sessions")

        def destroy(self):
            count("sessions_destroyed")

    class Engine:
        def __init__(self, device=0, rank=0):
            self.rank = rank
            count("engines")

        @classmethod
        def loopback(cls, session, rank, device=0):
            return cls(device, rank)

        def destroy(self):
            count("engines_destroyed")

    return types.SimpleNamespace(Engine=Engine, LoopbackSession=Session), log


@pytest.mark.parametrize("world", [1, 3])
def test_run_ranks_returns_every_ranks_value(world):
    mv, log = _fake()
    out = run_ranks(world, lambda r, e: (r, e.rank), _mv=mv)
    assert out == {r: (r, r) for r in range(world)}
    assert log.engines == log.engines_destroyed == world
    assert log.sessions == log.sessions_destroyed == int(world > 1)


def test_run_ranks_names_every_rank_that_raised():
    mv, log = _fake()

    def body(r, e):
        if r != 1:
            raise ValueError(f"boom {r}")
        return r

    with pytest.raises(AssertionError) as ex:
        run_ranks(3, body, _mv=mv)
    assert "[0, 2]" in str(ex.value)
    assert "boom 0" in str(ex.value) and "boom 2" in str(ex.value)
    assert log.sessions_destroyed == 1 and log.engines_destroyed == 3


def test_run_ranks_leaks_the_session_of_a_hung_rank_and_ends_pytest():
    mv, log = _fake()
    release = threading.Event()

    def body(r, e):
        if r == 1:
            release.wait(30)
        return r

    try:
        with pytest.raises(pytest.exit.Exception) as ex:
            run_ranks(2, body, join_s=0.05, _mv=mv)
        assert ex.value.returncode not in (0, None)
        assert "[1]" in str(ex.value)
        assert log.sessions == 1 and log.sessions_destroyed == 0
    finally:
        release.set()
