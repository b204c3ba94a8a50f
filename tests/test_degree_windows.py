"""The windowed degree order (mv_degree_window_order), on the host.

The engine folds this order into its internal layout at graph load so that
every SELL slice of 64 vertices holds nearly equal degrees. It is layout
only; what has to hold is the placement rule itself, restated here in numpy:
per aligned window of W positions, a stable sort by (deg + q - 1) // q,
descending, cut into rows of 64; with R = W/64 rows and G = R/S groups the
sorted row r lands at row (r mod G)*S + r//G; a short last window stays
plainly sorted.
"""
import numpy as np
import pytest

from minivite_amd import Graph, degree_window_order

CASES = [(128, 1, 1), (128, 1, 2), (512, 4, 2), (512, 1, 8), (16384, 1, 8),
         (32768, 2, 8)]


def _rule(hint, xadj, W, q, S):
    lnv = len(xadj) - 1
    hint = np.arange(lnv, dtype=np.int32) if hint is None else hint
    deg = np.diff(xadj)
    out = np.empty(lnv, dtype=np.int32)
    R, G = W // 64, W // 64 // S
    for b in range(0, lnv, W):
        win = hint[b:b + W]
        key = (deg[win] + q - 1) // q
        srt = win[np.argsort(-key, kind="stable")]
        if len(win) == W and G > 1:
            rows = srt.reshape(R, 64)
            placed = np.empty_like(rows)
            r = np.arange(R)
            placed[(r % G) * S + r // G] = rows
            srt = placed.reshape(-1)
        out[b:b + len(win)] = srt
    return out


def _padded_entries(order, xadj):
    deg = np.diff(xadj)[order]
    pad = (-len(deg)) % 64
    rows = np.concatenate([deg, np.zeros(pad, dtype=deg.dtype)])
    return int(64 * rows.reshape(-1, 64).max(axis=1).sum())


def _rgg():
    g = Graph.rgg(16384)
    try:
        return g.locality_hint(), g.arrays()[0]
    finally:
        g.free()


def _handmade():
    """lnv = 130, degrees 0..12, no hint (identity): one full window of 128
    plus a short one of 2 at W = 128, a single short window above."""
    deg = (np.arange(130) * 7) % 13
    assert set(deg) == set(range(13))
    return None, np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


@pytest.fixture(scope="module", params=["rgg16384", "handmade130"])
def graph(request):
    return _rgg() if request.param == "rgg16384" else _handmade()


@pytest.mark.parametrize("W,q,S", CASES)
def test_order_follows_the_rule(graph, W, q, S):
    hint, xadj = graph
    lnv = len(xadj) - 1
    got = degree_window_order(hint, xadj, W, q, S)
    assert got.dtype == np.int32 and got.shape == (lnv,)
    assert np.array_equal(got, _rule(hint, xadj, W, q, S))
    # a permutation
    assert np.array_equal(np.sort(got), np.arange(lnv))
    # no vertex leaves its window
    base = np.arange(lnv, dtype=np.int32) if hint is None else hint
    for b in range(0, lnv, W):
        assert np.array_equal(np.sort(got[b:b + W]), np.sort(base[b:b + W]))
    # the SELL image never grows
    assert _padded_entries(got, xadj) <= _padded_entries(base, xadj)


def test_rgg_hint_is_present_and_shrinks():
    """The n=16384 RGG carries a hint, and the order pays on it: the padded
    entry count falls by more than a tenth at W = 512."""
    hint, xadj = _rgg()
    assert hint is not None
    got = degree_window_order(hint, xadj, 512, 1, 8)
    assert _padded_entries(got, xadj) < 0.9 * _padded_entries(hint, xadj)


@pytest.mark.parametrize("W,q,S", [(0, 1, 1), (64, 1, 1), (192, 1, 1),
                                   (128, 0, 1), (128, 1, 4), (512, 1, 3)])
def test_bad_arguments_are_refused(W, q, S):
    _, xadj = _handmade()
    with pytest.raises(ValueError):
        degree_window_order(None, xadj, W, q, S)
