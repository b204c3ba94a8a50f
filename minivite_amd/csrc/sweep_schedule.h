// sweep_schedule.h — the integer arithmetic behind the sweep's row schedule,
// as plain host functions (no HIP): the engine decides with them at graph
// load and at every queued launch, and mv_sweep_schedule (graph_build.cpp)
// hands the same functions to the CPU tests. Not part of the C-ABI.
#ifndef MINIVITE_SWEEP_SCHEDULE_H
#define MINIVITE_SWEEP_SCHEDULE_H

#include <algorithm>
#include <cstdint>

constexpr int QUEUE_HEADS = 8; // ticket words (one per XCD)

// Largest default queue unit (rows) of the general sweep: the best cell of
// the measured U x grid table (experiments/RESULTS.md, "row queue").
constexpr int SWEEP_UNIT_DEFAULT = 4;

// Default row-group length S of a graph of lnv vertices under a degree
// window of W vertices, for a sweep grid of `grid` blocks of four waves: the
// largest power of two <= min(W/64, rows per wave), or 0 (degree windows off)
// where that is below 2 — a row per wave at most: keep every wave busy.
inline int64_t default_row_group(int64_t lnv, int grid, int64_t W) {
    const int64_t rows = (lnv + 63) / 64;
    const int64_t waves = 4 * (int64_t)grid;
    const int64_t cap = std::min(W / 64, (rows + waves - 1) / waves);
    int64_t S = 1;
    while (S * 2 <= cap) S *= 2;
    return S < 2 ? 0 : S;
}

// Default queue unit U (rows): at least two units per wave of the grid, or
// the queue has nothing to do — the largest of 4, 2, else 0 (static).
inline int default_sweep_unit(int64_t lnv, int grid) {
    const int64_t rows = (lnv + 63) / 64;
    const int64_t per_wave = rows / (4 * (int64_t)grid);
    int U = SWEEP_UNIT_DEFAULT;
    for (; U > 2 && 2 * U > per_wave; U /= 2) {}
    return 2 * U > per_wave ? 0 : U;
}

// A queued launch over `positions` SELL positions in units of `unit` rows on
// `grid` blocks: returns the ticket words in use (a power of two <= blocks)
// and sets add[h], h < heads, to the tickets the launch takes from head h —
// nu in all, a ticket per unit (see RowQueue in sweep.hip).
inline int queue_tickets(int64_t positions, int unit, int grid,
                         int64_t add[QUEUE_HEADS]) {
    int heads = 1;
    while (heads * 2 <= std::min(grid, QUEUE_HEADS)) heads *= 2;
    const int64_t H = heads;
    const int64_t rows = (positions + 63) / 64;
    const int64_t nu = (rows + unit - 1) / unit, nw = 4 * (int64_t)grid;
    const int64_t nq = std::max<int64_t>(nu - nw, 0); // queued units
    const int64_t m = std::min(nu, nw); // waves with a first unit: each
                                        // ends on one dry ticket
    auto share = [H](int64_t n, int64_t h) { // |{j < n : j % H == h}|
        return n > h ? (n - h + H - 1) / H : 0;
    };
    for (int64_t h = 0; h < H; h++)
        add[h] = share(nq, h) + 4 * share(m / 4, h) +
                 ((m / 4) % H == h ? m % 4 : 0);
    return heads;
}

#endif
