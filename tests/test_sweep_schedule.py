"""The defaults of the sweep's row schedule, on the CPU.

choose_row_queue and choose_degree_windows (engine.hip) take the queue unit U
and the row-group length S of a graph from two host functions in
sweep_schedule.h; mv_sweep_schedule hands the same functions to this test,
which needs no GPU. The rules, as DESIGN.md states them (a wave is a quarter
of a 256-thread block, a row 64 positions):

  U: at least two units per wave of the sweep grid -- the largest of 4 and
     2 with 2U <= floor(rows / waves), else 0 (static schedule);
  S: the largest power of two <= min(W/64, rows per wave), rows per wave =
     ceil(rows / waves); below 2 the windowed order is off (0 here).

The expected values of the named shapes are the ones the GPU tests assert
(test_gpu_sweep_queue.py::test_default_unit*, test_gpu_degree_windows.py).
"""
import pytest

from minivite_amd import sweep_schedule

W_DEFAULT = 2048


def _rows(lnv):
    return (lnv + 63) // 64


def rule_unit(lnv, grid):
    per_wave = _rows(lnv) // (4 * grid)
    for U in (4, 2):
        if 2 * U <= per_wave:
            return U
    return 0


def rule_row_group(lnv, grid, W):
    waves = 4 * grid
    cap = min(W // 64, -(-_rows(lnv) // waves))
    S = 1
    while S * 2 <= cap:
        S *= 2
    return S if S >= 2 else 0


@pytest.mark.parametrize("lnv,grid,U", [
    (1 << 22, 2048, 4),    # the bench shape: 8 rows per wave
    (1 << 21, 2048, 2),    # test_default_unit: 4 rows per wave
    (16384, 64, 0),        # ... and its small graph: one row per wave
    (16384, 8, 4),         # test_default_unit_four_on_a_capped_grid
    (8192, 8, 2),          # a rank of two on the capped grid: 4 per wave
    (1, 1, 0),
])
def test_default_unit_of_the_named_shapes(lnv, grid, U):
    assert sweep_schedule(lnv, grid)[0] == U
    assert rule_unit(lnv, grid) == U


@pytest.mark.parametrize("grid", [1, 3, 8])
@pytest.mark.parametrize("per_wave,U", [
    (0, 0), (1, 0), (3, 0),   # 2U - 1 for U = 2: off
    (4, 2),                   # 2U for U = 2
    (7, 2),                   # 2U - 1 for U = 4: still 2
    (8, 4),                   # 2U for U = 4
    (9, 4), (1000, 4),        # never more than 4
])
def test_default_unit_thresholds(per_wave, U, grid):
    waves = 4 * grid
    # floor(rows / waves) == per_wave from its first row count to its last,
    # a partial last row included
    for rows in (per_wave * waves, per_wave * waves + waves - 1):
        for lnv in (64 * rows, max(64 * rows - 63, 0)):
            if _rows(lnv) != rows:
                continue
            assert sweep_schedule(lnv, grid)[0] == U, (rows, lnv)
            assert rule_unit(lnv, grid) == U


@pytest.mark.parametrize("lnv,grid,W,S", [
    (1 << 22, 2048, W_DEFAULT, 8),  # the bench shape: 8 rows per wave
    (1 << 21, 2048, W_DEFAULT, 4),
    (16384, 64, W_DEFAULT, 0),      # test_default_routing_leaves_small_...
    (16384, 8, W_DEFAULT, 8),       # a capped grid: 8 rows per wave
    (16384, 8, 128, 2),             # the window holds two rows
    (16384, 8, 256, 4),
    (1 << 24, 2048, W_DEFAULT, 32), # 32 rows per wave: W/64 = 32 rows
    (1 << 25, 2048, W_DEFAULT, 32), # more rows than the window has
    (1, 1, W_DEFAULT, 0),
])
def test_default_row_group_of_the_named_shapes(lnv, grid, W, S):
    assert sweep_schedule(lnv, grid, window=W)[1] == S
    assert rule_row_group(lnv, grid, W) == S


@pytest.mark.parametrize("grid", [1, 3, 8])
@pytest.mark.parametrize("rows_per_wave,extra,S", [
    (1, 0, 0),     # exactly one row per wave: off
    (1, 1, 2),     # one row more: some wave has two
    (2, 0, 2),     # exactly two rows per wave
    (3, 0, 2), (3, 1, 4), (4, 0, 4), (7, 1, 8), (8, 0, 8), (8, 1, 8),
    (16, 1, 16),
])
def test_default_row_group_thresholds(rows_per_wave, extra, S, grid):
    rows = rows_per_wave * 4 * grid + extra
    for lnv in (64 * rows, 64 * rows - 63):
        assert sweep_schedule(lnv, grid, window=W_DEFAULT)[1] == S, lnv
        assert rule_row_group(lnv, grid, W_DEFAULT) == S
    # the window caps it: W = 128 holds two rows
    want = min(S, 2)
    assert sweep_schedule(64 * rows, grid, window=128)[1] == want


def test_rule_and_library_agree_on_a_sweep():
    for grid in (1, 2, 5, 64, 2048):
        for rows in list(range(0, 70)) + [4 * grid * k + d for k in (1, 2, 4, 8)
                                          for d in (-1, 0, 1)]:
            lnv = 64 * max(rows, 0)
            for W in (128, 512, W_DEFAULT):
                U, S, _ = sweep_schedule(lnv, grid, window=W)
                assert U == rule_unit(lnv, grid), (lnv, grid)
                assert S == rule_row_group(lnv, grid, W), (lnv, grid, W)


def test_bad_arguments_are_refused():
    for kw in ({"lnv": -1}, {"sweep_grid": 0}, {"window": -1},
               {"positions": -1}, {"unit": 0}, {"launch_grid": 0}):
        args = {"lnv": 64, "sweep_grid": 1, **kw}
        with pytest.raises(ValueError):
            sweep_schedule(**args)
