// multiphase.hip — phase assignment + the multi-phase driver (DESIGN.md,
// multi-phase section): the distributed aggregation over engine.hip's
// transport seam and coarsen.hip's kernels, and the one phase loop. The
// reference mini-app stops after phase one: no counterpart there.

#include <cmath>
#include <memory>

#include "coarsen.h"
#include "engine_internal.h"

struct mv_hierarchy {
    std::vector<mv_graph *> graphs;     // [0] unused (the caller's graph)
    std::vector<std::vector<i64>> maps; // [0] unused
    std::vector<double> q;              // levels 0..L
    std::vector<mv_phase_info> info;    // phases 1..P at [0..P)
    std::vector<i64> prop_nv;           // what each phase proposed
    std::vector<double> prop_q;
    std::vector<i64> comm;              // nv0 dense ids
    ~mv_hierarchy() {
        for (auto *g : graphs)
            if (g) mv_graph_free(g);
    }
};

static const int kMaxPhases = 64; // every kept level has fewer vertices
                                  // than the one before; RGG 2^22 needs 9

// ------------------------------------------------------------------------
// Distributed aggregation (multi-phase section): the level is
// split by `parts`, every rank holds its slice, and the coarse level comes
// out split evenly. The exchanges below call the transport seam directly
// (not run_halo1a), so the halo counters keep describing the last run. The
// kernels and the sort / run-reduction pipeline are coarsen.hip's.

// count allgather that also serves nranks == 1 (no communicator there)
static void gather_counts(mv_engine *e, const i64 *mine, i64 *matrix) {
    if (e->nranks == 1) {
        matrix[0] = mine[0];
        return;
    }
    allgather_counts(e, mine, /*on_device*/ false, matrix, e->comm,
                     e->stream);
}

// true on every rank when any rank raised `bad`
static bool any_rank(mv_engine *e, bool bad) {
    const int p = e->nranks;
    std::vector<i64> mine(p, bad ? 1 : 0), m((size_t)p * p);
    gather_counts(e, mine.data(), m.data());
    for (int r = 0; r < p; r++)
        if (m[(size_t)r * p]) return true;
    return false;
}

// alltoallv of 8-byte elements (ids, keys, or the bit patterns of doubles)
static void a2a64(mv_engine *e, const void *send, const i64 *soff, void *recv,
                  const i64 *roff) {
    if (e->nranks == 1) return;
    alltoallv(e, send, soff, recv, roff, 8, ncclInt64, e->comm, e->stream);
}

// d_vals[k] = the owner's table entry of d_uniq[k]: d_uniq holds sorted
// distinct global ids of a level split by parts, d_table one value per
// vertex this rank owns. Requests are bucketed by owner, counted, sent,
// gathered at the owner and sent back. Collective; synchronises.
static void dist_fetch(mv_engine *e, const i64 *parts, const i64 *d_uniq,
                       i64 nuniq, const i64 *d_table, i64 *d_vals) {
    const int p = e->nranks, me = e->rank;
    hipStream_t st = e->stream;
    std::vector<uint64_t> keys(parts, parts + p + 1);
    std::vector<i64> soff(p + 1), roff, cnt(p), m((size_t)p * p);
    mv_lower_bounds(st, (const uint64_t *)d_uniq, nuniq, keys.data(), p + 1,
                    soff.data());
    for (int r = 0; r < p; r++) cnt[r] = soff[r + 1] - soff[r];
    gather_counts(e, cnt.data(), m.data());
    recv_offsets(m, p, me, /*with_own*/ false, roff);
    const i64 nreq = roff[p];
    DevBuf<i64> d_req(nreq), d_rep(nreq);
    a2a64(e, d_uniq, soff.data(), d_req, roff.data());
    mv_gather_owned(st, nreq, d_req, parts[me], d_table, d_rep);
    mv_gather_owned(st, cnt[me], d_uniq + soff[me], parts[me], d_table,
                    d_vals + soff[me]); // my own segment stays home
    a2a64(e, d_rep, roff.data(), d_vals, soff.data());
    HIP_CHECK(hipStreamSynchronize(st));
}

// d_out[i] = the owner's table entry of d_ids[i], i < n (ids of a level
// of nv vertices split by parts): sort-unique, fetch, scatter back through
// the sort permutation. Collective; synchronises.
static void dist_lookup(mv_engine *e, const i64 *parts, i64 nv,
                        const i64 *d_ids, i64 n, const i64 *d_table,
                        i64 *d_out) {
    mv_unique_ids u;
    mv_sort_unique_ids(e->stream, n, d_ids, ceil_log2(nv), &u);
    DevBuf<i64> d_vals(u.nuniq);
    dist_fetch(e, parts, u.d_uniq, u.nuniq, d_table, d_vals);
    mv_scatter_unique(e->stream, &u, d_vals, d_out);
    HIP_CHECK(hipStreamSynchronize(e->stream));
}

// this rank's slice of a coarse level, on the device
struct DistCoarse {
    i64 nc = 0, lnc = 0, ne = 0;
    std::vector<i64> parts; // the even split of nc
    DevBuf<i64> d_map;      // lnv: global dense coarse id per local vertex
    DevBuf<i64> d_xadj, d_tails; // lnc+1 (local offsets), ne (global tails)
    DevBuf<double> d_w;
};

static const i64 kCubItems = (1ll << 31) - 1; // hipCUB item counts are int

// Aggregate the slice (device CSR, global tails; d_w null = unit weights)
// by d_labels. `bad` is this rank's own verdict on its input; together
// with the nv / local-edge limits and the label range it travels in the
// first count allgather, so that every rank returns non-zero when one
// does (the received-partials limit is judged by every rank from the
// redistribution's count matrix: collective as well). With
// stop_if_identity a labelling that merges nothing (nc == nv, globally)
// returns after the renumbering. Collective; synchronises.
static int coarsen_dist_device(mv_engine *e, const i64 *parts, i64 nv,
                               i64 lnv, i64 lne, const i64 *d_xadj,
                               const i64 *d_tails, const double *d_w,
                               const i64 *d_labels, bool bad,
                               bool stop_if_identity, DistCoarse *out) {
    const int p = e->nranks, me = e->rank;
    hipStream_t st = e->stream;
    // a slice the caller already refused may not even have my parts entries
    // (built for fewer ranks): they are read only for a sound one
    const i64 base = bad ? 0 : parts[me], bound = bad ? 0 : parts[me + 1];
    const int bits = ceil_log2(nv);
    std::vector<i64> soff(p + 1, 0), roff, cnt(p), m((size_t)p * p);
    std::vector<uint64_t> keys(p + 1);

    // ---- (a) renumber: distinct labels to their owners ----
    if (nv < 1 || nv >= (1ll << 31) || lne >= kCubItems) {
        std::fprintf(stderr,
                     "coarsen (rank %d): need 1 <= nv < 2^31 and local edges "
                     "< 2^31 - 1 (nv=%lld lne=%lld)\n",
                     me, (long long)nv, (long long)lne);
        bad = true;
    }
    mv_unique_ids u;
    if (!bad) {
        DevBuf<i64> d_lab(lnv);
        DevBuf<unsigned> d_err(1);
        HIP_CHECK(hipMemsetAsync(d_err, 0, 4, st));
        mv_check_labels(st, lnv, d_labels, nv, d_lab, d_err);
        if (read_back(d_err.get(), st)) {
            std::fprintf(stderr,
                         "coarsen (rank %d): community label outside "
                         "[0, nv=%lld)\n",
                         me, (long long)nv);
            bad = true;
        } else {
            mv_sort_unique_ids(st, lnv, d_lab, bits, &u);
            for (int r = 0; r <= p; r++) keys[r] = (uint64_t)parts[r];
            mv_lower_bounds(st, (const uint64_t *)u.d_uniq.get(), u.nuniq,
                            keys.data(), p + 1, soff.data());
        }
    }
    for (int r = 0; r < p; r++) cnt[r] = bad ? -1 : soff[r + 1] - soff[r];
    gather_counts(e, cnt.data(), m.data());
    for (size_t k = 0; k < m.size(); k++)
        if (m[k] < 0) // some rank refused: everyone does, before any send
            return -1;
    recv_offsets(m, p, me, /*with_own*/ false, roff);
    i64 nc = 0, offset = 0;
    DevBuf<i64> d_dense; // dense coarse id of every owned label in use
    {
        const i64 nreq = roff[p];
        DevBuf<i64> d_req(nreq);
        DevBuf<unsigned> d_used(lnv + 1), d_rank(lnv + 1);
        a2a64(e, u.d_uniq, soff.data(), d_req, roff.data());
        HIP_CHECK(hipMemsetAsync(d_used, 0, 4 * (lnv + 1), st));
        mv_mark_owned(st, nreq, d_req, base, d_used);
        mv_mark_owned(st, cnt[me], u.d_uniq + soff[me], base, d_used);
        mv_exclusive_sum_u32(st, d_used, d_rank, lnv + 1);
        std::vector<i64> mine(p, (i64)read_back(d_rank + lnv, st));
        gather_counts(e, mine.data(), m.data());
        for (int r = 0; r < p; r++) {
            if (r < me) offset += m[(size_t)r * p];
            nc += m[(size_t)r * p];
        }
        d_dense.reserve(lnv);
        mv_dense_ids(st, lnv, d_rank, offset, d_dense);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    out->d_map.reserve(lnv);
    {
        DevBuf<i64> d_vals(u.nuniq);
        dist_fetch(e, parts, u.d_uniq, u.nuniq, d_dense, d_vals);
        mv_scatter_unique(st, &u, d_vals, out->d_map);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    out->nc = nc;
    out->parts.resize(p + 1);
    for (int r = 0; r <= p; r++) out->parts[r] = (nc * r) / p;
    out->lnc = out->parts[me + 1] - out->parts[me];
    if (stop_if_identity && nc == nv) return 0;

    // ---- (b) coarse ids of the tails: remote ones are fetched; then the
    // keys, local sort + run reduction: one partial per local pair ----
    const int shift = ceil_log2(nc);
    mv_key_runs part;
    {
        DevBuf<i64> d_gids; // the distinct remote tails, sorted
        const i64 ngh = remote_ids(st, lne, d_tails, base, bound, bits, d_gids);
        DevBuf<i64> d_gmap(ngh);
        dist_fetch(e, parts, d_gids, ngh, out->d_map, d_gmap);
        DevBuf<uint64_t> d_keys(lne);
        mv_coarse_keys_dist(st, lnv, lne, d_xadj, d_tails, base, bound,
                            out->d_map, d_gids, ngh, d_gmap, shift, d_keys);
        mv_sort_reduce_keys(st, lne, d_keys, d_w, 2 * shift, &part);
    }

    // ---- redistribution: every partial to the owner of its row ----
    for (int r = 0; r <= p; r++)
        keys[r] = (uint64_t)out->parts[r] << shift;
    mv_lower_bounds(st, part.d_key, part.n, keys.data(), p + 1, soff.data());
    for (int r = 0; r < p; r++) cnt[r] = soff[r + 1] - soff[r];
    gather_counts(e, cnt.data(), m.data());
    for (int q = 0; q < p; q++) { // every rank checks every rank's total
        i64 tot = 0;
        for (int r = 0; r < p; r++) tot += m[(size_t)r * p + q];
        if (tot >= kCubItems) {
            std::fprintf(stderr,
                         "coarsen (rank %d): rank %d would receive %lld "
                         "partial edges, need < 2^31 - 1\n",
                         me, q, (long long)tot);
            return -1;
        }
    }
    // segments by ascending sender, my own in its place: the stable sort
    // then adds the per-rank partials of a pair in rank order
    recv_offsets(m, p, me, /*with_own*/ true, roff);
    const i64 nrecv = roff[p];
    mv_key_runs fin;
    {
        DevBuf<uint64_t> d_rk(nrecv);
        DevBuf<double> d_rw(nrecv);
        if (cnt[me] > 0) {
            HIP_CHECK(hipMemcpyAsync(d_rk + roff[me], part.d_key + soff[me],
                                     8 * cnt[me], hipMemcpyDeviceToDevice,
                                     st));
            HIP_CHECK(hipMemcpyAsync(d_rw + roff[me], part.d_w + soff[me],
                                     8 * cnt[me], hipMemcpyDeviceToDevice,
                                     st));
        }
        a2a64(e, part.d_key, soff.data(), d_rk, roff.data());
        a2a64(e, part.d_w, soff.data(), d_rw, roff.data());
        // ---- owner: stable sort of the segments, run reduction ----
        mv_sort_reduce_keys(st, nrecv, d_rk, d_rw, 2 * shift, &fin);
    }
    out->ne = fin.n;
    out->d_xadj.reserve(out->lnc + 1);
    out->d_tails.reserve(fin.n);
    mv_coarse_rows(st, out->parts[me], out->lnc, fin.n, shift, fin.d_key,
                   out->d_xadj, out->d_tails);
    HIP_CHECK(hipStreamSynchronize(st));
    out->d_w = std::move(fin.d_w); // the run weights ARE the coarse weights
    return 0;
}

// fill a host vector from the device (nothing for an empty one)
template <class T> static void to_host(std::vector<T> &h, const T *d) {
    if (!h.empty())
        HIP_CHECK(hipMemcpy(h.data(), d, sizeof(T) * h.size(),
                            hipMemcpyDeviceToHost));
}

// the coarse slice as a host level (parts = the even split)
static mv_graph *level_from_device(mv_engine *e, const DistCoarse &c) {
    std::vector<i64> cx(c.lnc + 1), ct(c.ne);
    std::vector<double> cw(c.ne);
    to_host(cx, c.d_xadj.get());
    to_host(ct, c.d_tails.get());
    to_host(cw, c.d_w.get());
    return mv_graph_from_csr(c.nc, e->rank, e->nranks, c.parts.data(), c.lnc,
                             c.ne, cx.data(), ct.data(), cw.data());
}

// q of a partitioned level: per-rank (selfloops, deg^2, W) in row order,
// reduced in rank order — the same bits, hence the same keep / drop / stop
// decision, on every rank. Collective at nranks > 1.
static double level_modularity_dist(mv_engine *e, const mv_graph *g) {
    const i64 lnv = mv_graph_lnv(g), base = mv_graph_parts(g)[e->rank];
    const i64 *xadj = mv_graph_xadj(g), *tails = mv_graph_tails(g);
    const double *w = mv_graph_weights(g);
    double red[3] = {0.0, 0.0, 0.0}; // loops, deg2, W
    for (i64 v = 0; v < lnv; v++) {
        double d = 0.0;
        for (i64 k = xadj[v]; k < xadj[v + 1]; k++) {
            d += w[k];
            if (tails[k] == base + v) red[0] += w[k];
        }
        red[2] += d;
        red[1] += d * d;
    }
    if (e->nranks > 1) comm_allreduce_host(e, red, 3);
    return red[2] == 0.0 ? 0.0 : red[0] / red[2] - red[1] / (red[2] * red[2]);
}

// host-side sanity of a caller's slice against this engine's rank
static bool slice_is_bad(const mv_engine *e, const mv_graph *g,
                         const char *who) {
    const i64 nv = mv_graph_nv(g), lnv = mv_graph_lnv(g),
              lne = mv_graph_lne(g);
    const i64 *parts = mv_graph_parts(g), *xadj = mv_graph_xadj(g),
              *tails = mv_graph_tails(g);
    if (mv_graph_nranks(g) != e->nranks || mv_graph_rank(g) != e->rank) {
        std::fprintf(stderr,
                     "%s (rank %d of %d): the graph is the slice of rank %d "
                     "of %d\n",
                     who, e->rank, e->nranks, mv_graph_rank(g),
                     mv_graph_nranks(g));
        return true;
    }
    bool bad = parts[0] != 0 || parts[e->nranks] != nv ||
               parts[e->rank + 1] - parts[e->rank] != lnv || xadj[0] != 0 ||
               xadj[lnv] != lne;
    for (int r = 0; r < e->nranks && !bad; r++) bad = parts[r] > parts[r + 1];
    for (i64 v = 0; v < lnv && !bad; v++) bad = xadj[v] > xadj[v + 1];
    for (i64 k = 0; k < lne && !bad; k++) bad = tails[k] < 0 || tails[k] >= nv;
    if (bad)
        std::fprintf(stderr,
                     "%s (rank %d): the graph is not this rank's slice of a "
                     "%d-rank partition (parts, xadj or a tail out of "
                     "range)\n",
                     who, e->rank, e->nranks);
    return bad;
}

// ------------------------------------------------------------------------
// The multi-phase driver: one phase loop behind both entry points. The
// aggregation and the final composition of the maps have a single-rank and
// a distributed arm; the rest is the distributed form, exact at one rank.
static mv_hierarchy *run_phases(mv_engine *e, const mv_graph *g, double lower,
                                double thresh, int max_phases) {
    HIP_CHECK(hipSetDevice(e->device));
    const int p = e->nranks;
    const int cap = max_phases >= 1 ? max_phases : kMaxPhases;
    std::unique_ptr<mv_hierarchy> h(new mv_hierarchy);
    h->graphs.push_back(nullptr);
    h->maps.emplace_back();
    h->q.push_back(level_modularity_dist(e, g));
    const mv_graph *cur = g;
    std::vector<i64> mine(p), m((size_t)p * p);
    for (int phase = 1; phase <= cap; phase++) {
        // nv >= 2^31 is the one refusal of a load: global, so collective
        if (mv_engine_load_graph(e, cur) != 0) return nullptr;
        mv_phase_info pi{};
        pi.nv_in = e->nv;
        std::fill(mine.begin(), mine.end(), e->lne);
        gather_counts(e, mine.data(), m.data());
        for (int r = 0; r < p; r++) pi.ne_in += m[(size_t)r * p];
        auto t0 = clk::now();
        pi.run_mod = mv_engine_run(e, lower, thresh, &pi.iters);
        pi.run_ms = ms_since(t0);
        h->info.push_back(pi);
        h->prop_nv.push_back(pi.nv_in);
        h->prop_q.push_back(h->q.back());
        mv_phase_info &info = h->info.back();

        // aggregate straight off the CSR the engine holds on the device:
        // nc, this rank's slice of the map and of the new level (or null)
        t0 = clk::now();
        i64 nc;
        std::vector<i64> map;
        mv_graph *ng;
        if (p == 1) {
            mv_coarse_dev c;
            if (mv_coarsen_device(e->stream, e->lnv, e->lne, e->d_xadj,
                                  e->d_tails,
                                  e->unit_weights ? nullptr : e->d_ew.get(),
                                  phase_labels_device(e),
                                  /*stop_if_identity*/ true, &c) != 0)
                return nullptr;
            if (c.nc == e->lnv) break; // no merge: the hierarchy is complete
            const double dev_ms = ms_since(t0); // the kernels, synchronised
            map.resize(e->lnv);
            std::vector<i64> cx(c.nc + 1), ct(c.ne);
            std::vector<double> cw(c.ne);
            to_host(map, c.d_map.get());
            to_host(cx, c.d_xadj.get());
            to_host(ct, c.d_tails.get());
            to_host(cw, c.d_w.get());
            const double copy_ms = ms_since(t0) - dev_ms;
            const i64 parts[2] = {0, c.nc};
            nc = c.nc;
            ng = mv_graph_from_csr(c.nc, 0, 1, parts, c.nc, c.ne, cx.data(),
                                   ct.data(), cw.data());
            info.coarsen_ms = ms_since(t0);
            if (getenv("MV_COARSEN_DEBUG"))
                std::fprintf(stderr,
                             "[coarsen] phase %d: device %.3f ms, D2H %.3f "
                             "ms, host level build %.3f ms\n",
                             phase, dev_ms, copy_ms,
                             info.coarsen_ms - dev_ms - copy_ms);
        } else {
            DistCoarse c; // collective, a refusal included
            if (coarsen_dist_device(e, e->parts_h.data(), e->nv, e->lnv,
                                    e->lne, e->d_xadj, e->d_tails,
                                    e->unit_weights ? nullptr : e->d_ew.get(),
                                    phase_labels_device(e), /*bad*/ false,
                                    /*stop_if_identity*/ true, &c) != 0)
                return nullptr;
            if (c.nc == e->nv) break; // no merge anywhere: complete
            nc = c.nc;
            map.resize(e->lnv);
            to_host(map, c.d_map.get());
            ng = level_from_device(e, c);
            info.coarsen_ms = ms_since(t0);
        }
        if (any_rank(e, ng == nullptr)) {
            if (ng) mv_graph_free(ng);
            return nullptr;
        }
        const double qn = level_modularity_dist(e, ng);
        h->prop_nv.back() = nc;
        h->prop_q.back() = qn;
        if (qn < h->q.back()) { // the proposal lowers q: drop it
            mv_graph_free(ng);
            break;
        }
        info.kept = 1;
        const double gain = qn - h->q.back();
        h->graphs.push_back(ng);
        h->maps.push_back(std::move(map));
        h->q.push_back(qn);
        cur = ng;
        if (gain < thresh) break;
    }
    // final communities: the maps composed. One rank (or no kept level)
    // walks them on the host; otherwise one distributed lookup per kept
    // level (level k's map is a table over level k-1's owners)
    const i64 lnv0 = mv_graph_lnv(g);
    h->comm.resize(lnv0);
    if (p == 1 || h->maps.size() == 1) {
        const i64 base = mv_graph_parts(g)[e->rank];
        for (i64 v = 0; v < lnv0; v++) {
            i64 c = base + v;
            for (size_t k = 1; k < h->maps.size(); k++) c = h->maps[k][c];
            h->comm[v] = c;
        }
    } else {
        DevBuf<i64> d_c, d_next, d_table;
        d_c.reserve(lnv0);
        d_next.reserve(lnv0);
        if (lnv0)
            HIP_CHECK(hipMemcpy(d_c, h->maps[1].data(), 8 * lnv0,
                                hipMemcpyHostToDevice));
        for (size_t k = 2; k < h->maps.size(); k++) {
            const mv_graph *lv = h->graphs[k - 1];
            const i64 n = (i64)h->maps[k].size();
            d_table.reserve(n);
            if (n)
                HIP_CHECK(hipMemcpy(d_table, h->maps[k].data(), 8 * n,
                                    hipMemcpyHostToDevice));
            dist_lookup(e, mv_graph_parts(lv), mv_graph_nv(lv), d_c, lnv0,
                        d_table, d_next);
            std::swap(d_c, d_next);
        }
        if (lnv0)
            HIP_CHECK(hipMemcpy(h->comm.data(), d_c, 8 * lnv0,
                                hipMemcpyDeviceToHost));
    }
    return h.release();
}

extern "C" {

int mv_engine_get_communities(mv_engine *e, int64_t *out) {
    HIP_CHECK(hipSetDevice(e->device));
    const i64 *lab = phase_labels_device(e);
    if (!lab) {
        std::fprintf(stderr, "mv_engine_get_communities: no run yet\n");
        return -1;
    }
    if (e->lnv) // a rank may own no vertices
        HIP_CHECK(hipMemcpyAsync(out, lab, 8 * e->lnv, hipMemcpyDeviceToHost,
                                 e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
    return 0;
}

mv_hierarchy *mv_engine_run_multiphase(mv_engine *e, const mv_graph *g,
                                       double lower, double thresh,
                                       int max_phases) {
    if (e->nranks > 1) {
        std::fprintf(stderr,
                     "mv_engine_run_multiphase: single-rank only (nranks=%d);"
                     " multi-rank coarsening needs an edge redistribution\n",
                     e->nranks);
        return nullptr;
    }
    if (mv_graph_lnv(g) != mv_graph_nv(g)) {
        std::fprintf(stderr,
                     "mv_engine_run_multiphase: graph is a multi-rank slice\n");
        return nullptr;
    }
    return run_phases(e, g, lower, thresh, max_phases);
}

mv_hierarchy *mv_engine_run_multiphase_dist(mv_engine *e, const mv_graph *g,
                                            double lower, double thresh,
                                            int max_phases) {
    HIP_CHECK(hipSetDevice(e->device));
    return any_rank(e, slice_is_bad(e, g, "mv_engine_run_multiphase_dist"))
               ? nullptr
               : run_phases(e, g, lower, thresh, max_phases);
}

mv_graph *mv_engine_coarsen_dist(mv_engine *e, const mv_graph *g,
                                 const int64_t *comm, int64_t *map_out) {
    HIP_CHECK(hipSetDevice(e->device));
    const bool bad = slice_is_bad(e, g, "mv_engine_coarsen_dist");
    const i64 nv = mv_graph_nv(g), lnv = bad ? 0 : mv_graph_lnv(g),
              lne = bad ? 0 : mv_graph_lne(g);
    const double *w = mv_graph_weights(g);
    bool unit = true;
    for (i64 k = 0; k < lne && unit; k++) unit = w[k] == 1.0;
    // the slice goes to buffers of its own: no run is behind this call and
    // the graph the engine holds stays loaded
    DevBuf<i64> d_xadj, d_tails, d_comm;
    DevBuf<double> d_w;
    d_xadj.reserve(lnv + 1);
    d_tails.reserve(lne);
    d_comm.reserve(lnv);
    if (!bad) {
        HIP_CHECK(hipMemcpy(d_xadj, mv_graph_xadj(g), 8 * (lnv + 1),
                            hipMemcpyHostToDevice));
        if (lne)
            HIP_CHECK(hipMemcpy(d_tails, mv_graph_tails(g), 8 * lne,
                                hipMemcpyHostToDevice));
        if (lnv)
            HIP_CHECK(hipMemcpy(d_comm, comm, 8 * lnv,
                                hipMemcpyHostToDevice));
        if (!unit) {
            d_w.reserve(lne);
            HIP_CHECK(hipMemcpy(d_w, w, 8 * lne, hipMemcpyHostToDevice));
        }
    }
    DistCoarse c;
    if (coarsen_dist_device(e, mv_graph_parts(g), nv, lnv, lne, d_xadj,
                            d_tails, unit ? nullptr : d_w.get(), d_comm, bad,
                            /*stop_if_identity*/ false, &c) != 0)
        return nullptr;
    if (lnv)
        HIP_CHECK(hipMemcpy(map_out, c.d_map, 8 * lnv,
                            hipMemcpyDeviceToHost));
    return level_from_device(e, c);
}

int mv_hierarchy_phases(const mv_hierarchy *h) { return (int)h->info.size(); }

int mv_hierarchy_levels(const mv_hierarchy *h) {
    return (int)h->graphs.size() - 1;
}

const mv_graph *mv_hierarchy_graph(const mv_hierarchy *h, int level) {
    return level >= 1 && level < (int)h->graphs.size() ? h->graphs[level]
                                                       : nullptr;
}

const int64_t *mv_hierarchy_map(const mv_hierarchy *h, int level) {
    return level >= 1 && level < (int)h->maps.size() ? h->maps[level].data()
                                                     : nullptr;
}

double mv_hierarchy_modularity(const mv_hierarchy *h, int level) {
    return level >= 0 && level < (int)h->q.size() ? h->q[level] : NAN;
}

int mv_hierarchy_phase_info(const mv_hierarchy *h, int phase,
                            mv_phase_info *out) {
    if (phase < 1 || phase > (int)h->info.size()) return -1;
    *out = h->info[phase - 1];
    return 0;
}

int mv_hierarchy_phase_proposal(const mv_hierarchy *h, int phase,
                                int64_t *nv_out, double *q_out) {
    if (phase < 1 || phase > (int)h->info.size()) return -1;
    *nv_out = h->prop_nv[phase - 1];
    *q_out = h->prop_q[phase - 1];
    return 0;
}

const int64_t *mv_hierarchy_communities(const mv_hierarchy *h) {
    return h->comm.data();
}

void mv_hierarchy_free(mv_hierarchy *h) { delete h; }

} // extern "C"
