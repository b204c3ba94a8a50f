"""The ticket arithmetic of the sweep's row queue, on the CPU.

k4_sweep's RowQueue: the rows of a launch are cut into units of U rows,
unit k = rows [kU, min((k+1)U, rows)). Wave x starts with unit x; the units
from `waves` on are queued on `heads` ticket words, head h = block & (heads
- 1), whose i-th ticket is queued unit i * heads + h. A wave stops at its
first unit past the end. The host (take_queue in sweep.hip, with the figures
of queue_tickets in sweep_schedule.h) advances a running total per head by
what the launch must consume and passes the old totals as bases; the words
are never reset.

This model plays the kernel's loop for any number of blocks in any arrival
order and checks: every row is walked exactly once and in order inside a
unit, and every head's word advances by exactly the host's figure, launch
after launch -- nu tickets per launch in all. The host's figure is restated
here (heads_for / host_tickets) and checked against the library's own
(mv_sweep_schedule), so the model vouches for the code that ships.
"""
import random

import pytest

from minivite_amd import sweep_schedule

QUEUE_HEADS = 8


def heads_for(grid):
    h = 1
    while h * 2 <= min(grid, QUEUE_HEADS):
        h *= 2
    return h


def host_tickets(rows, unit, grid):
    """Per head, what take_queue adds to tickets_total for one launch."""
    H = heads_for(grid)
    nu, nw = (rows + unit - 1) // unit, 4 * grid
    nq, m = max(nu - nw, 0), min(nu, nw)

    def share(n, h):  # |{j < n : j % H == h}|
        return (n - h + H - 1) // H if n > h else 0

    return [share(nq, h) + 4 * share(m // 4, h)
            + (m % 4 if (m // 4) % H == h else 0) for h in range(H)]


def play_launch(words, rows, unit, grid, rng):
    """row_first / row_next under a random interleaving of the waves.
    -> rows walked per wave, in walking order; `words` advances in place."""
    H = heads_for(grid)
    nw = 4 * grid
    base = [w & 0xFFFFFFFF for w in words]     # RowQueue::base: low words
    walked = [[] for _ in range(nw)]

    def enter(w, k):                           # unit_enter
        row = k * unit
        if row >= rows:
            return False
        walked[w].extend(range(row, min(row + unit, rows)))
        return True

    live = []
    order = list(range(nw))
    rng.shuffle(order)                         # waves start in any order
    pending = order
    while live or pending:
        if pending and (not live or rng.random() < 0.3):
            w = pending.pop()
            if enter(w, w):                    # row_first: unit = wave
                live.append(w)
            continue
        w = rng.choice(live)
        h = (w // 4) & (H - 1)                 # queue_take
        i = ((words[h] & 0xFFFFFFFF) - base[h]) & 0xFFFFFFFF
        words[h] += 1
        if not enter(w, nw + i * H + h):
            live.remove(w)
    return walked


CASES = [  # (positions, unit, blocks)
    (1, 2, 1), (63, 2, 1), (65, 2, 1), (130, 2, 1),   # the tiny GPU cases
    (16384, 1, 8), (16384, 3, 8), (16384, 8, 8),      # MV_SWEEP_GRID=8
    (16384, 1, 64), (16384, 3, 64), (16384, 8, 64),
    (8192, 3, 32), (8192, 8, 8), (70, 3, 1), (8122, 3, 5),  # a rank of two
    (4194304, 2, 1536), (4194304, 4, 1536), (4194304, 8, 2048),  # bench
    (2097152, 2, 1536), (100, 4096, 3), (64 * 7 + 1, 7, 1),
]


@pytest.mark.parametrize("positions,unit,grid", CASES)
def test_units_cover_rows_and_tickets_add_up(positions, unit, grid):
    rng = random.Random(positions * 131 + unit * 7 + grid)
    rows = (positions + 63) // 64
    nu = (rows + unit - 1) // unit
    # start near a 32-bit wrap of the never-reset words: only low words are
    # subtracted in the kernel
    words = [(1 << 32) - 3 - h for h in range(QUEUE_HEADS)]
    expected = list(words)
    for _ in range(3):                # launches are serial on one stream
        walked = play_launch(words, rows, unit, grid, rng)
        add = host_tickets(rows, unit, grid)
        assert sum(add) == nu         # a ticket per unit, however they fall
        for h, a in enumerate(add):
            expected[h] += a
        assert words == expected      # ... and head by head
        flat = sorted(r for w in walked for r in w)
        assert flat == list(range(rows))      # every row exactly once
        for w in walked:              # inside a unit rows ascend by one
            for a, b in zip(w, w[1:]):
                if a // unit == b // unit:
                    assert b == a + 1
        assert {r // unit for w in walked for r in w} == set(range(nu))


@pytest.mark.parametrize("positions,unit,grid", CASES)
def test_library_tickets_equal_the_model(positions, unit, grid):
    """queue_tickets, the function take_queue calls, against the copy the
    model above was checked with: head count, per-head additions, nu."""
    rows = (positions + 63) // 64
    _, _, add = sweep_schedule(positions, grid, positions=positions,
                               unit=unit, launch_grid=grid)
    assert len(add) == heads_for(grid)
    assert add == host_tickets(rows, unit, grid)
    assert sum(add) == (rows + unit - 1) // unit
