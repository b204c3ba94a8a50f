/* minivite_hip.h — C-ABI drop-in boundary of the MI355X-native miniVite
 * Louvain implementation.
 *
 * The reference's plugin surface is the distLouvainMethod call plus the
 * Graph accessors it consumes (caller: main.cpp:164-170; signature
 * dspl.hpp:1280-1284; Graph reads graph.hpp:140-203). The six comm-buffer
 * parameters of the reference signature are opaque scratch the caller only
 * declares (main.cpp:153-157) and are owned by the engine here. Each entry
 * point below cites the reference interface it replaces. See INTEGRATION.md
 * for the binding a maintainer would add to the reference's main.cpp.
 *
 * Process model: one process per GPU ("rank" == the reference's MPI rank;
 * "nranks" == its nprocs). Collectives ride RCCL over xGMI; rank 0 creates
 * the 128-byte RCCL unique id (mv_comm_id) and the caller transports it to
 * the other ranks (any side channel; bench.py uses a torch.distributed gloo
 * broadcast). Single-rank runs pass NULL.
 */
#ifndef MINIVITE_HIP_H
#define MINIVITE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- graph construction (replaces graph.hpp plumbing, host-side) ---- */

/* Per-rank partitioned CSR (replaces class Graph, graph.hpp:85-296).
 * Host memory; tails are GLOBAL vertex ids. */
typedef struct mv_graph mv_graph;

/* GenerateRGG::generate with isLCG=true (graph.hpp:584-1213 via the -l
 * path). Produces the BIT-IDENTICAL per-rank edge set using a cell-list
 * instead of the reference's O((nv/p)^2) pair loops; needs no
 * communication (the LCG stream is leapfrogged locally). Requirements as
 * the reference: nranks a power of two, nranks | nv, 1/nranks > rn
 * (graph.hpp:610-633). random_edge_percent > 0 mirrors the -p option
 * (graph.hpp:939-1122) except that the seed is explicit instead of
 * time(0)^getpid() (graph.hpp:990) and the O(n) duplicate scan
 * (graph.hpp:1013-1018) is not reproduced (perf configs only). */
mv_graph *mv_graph_rgg(int64_t nv, int rank, int nranks,
                       int unit_edge_weight, double random_edge_percent,
                       uint64_t random_edge_seed);

/* BinaryEdgeList::read / read_balanced (graph.hpp:315-412 / 416-572).
 * Single-node local file, plain pread instead of MPI-IO. */
mv_graph *mv_graph_read_binary(const char *path, int rank, int nranks,
                               int balanced);

/* Adopt caller-owned arrays (copied). parts has nranks+1 entries
 * (graph.hpp:112-113 layout); weights NULL means unit weights. */
mv_graph *mv_graph_from_csr(int64_t nv, int rank, int nranks,
                            const int64_t *parts, int64_t lnv, int64_t lne,
                            const int64_t *xadj, const int64_t *tails,
                            const double *weights);

/* Write this rank's slice of the reference's binary format is not needed;
 * mv_graph_write_binary writes a WHOLE single-rank graph (rank count 1)
 * to the reference .bin layout (graph.hpp:342-383) so the CPU reference
 * can consume framework-generated inputs via -f. */
int mv_graph_write_binary(const mv_graph *g, const char *path);

void mv_graph_free(mv_graph *g);

/* Accessors (graph.hpp:175-178 get_lnv/get_lne/get_nv + parts). */
int64_t mv_graph_nv(const mv_graph *g);
int64_t mv_graph_lnv(const mv_graph *g);
int64_t mv_graph_lne(const mv_graph *g);
const int64_t *mv_graph_parts(const mv_graph *g); /* nranks+1 */
/* The rank and rank count the slice was built for (no reference
 * counterpart: there the Graph shares the communicator's). */
int mv_graph_rank(const mv_graph *g);
int mv_graph_nranks(const mv_graph *g);
const int64_t *mv_graph_xadj(const mv_graph *g);  /* lnv+1 */
const int64_t *mv_graph_tails(const mv_graph *g); /* lne */
const double *mv_graph_weights(const mv_graph *g);/* lne */
/* Internal-layout hint (NULL if absent): locality_perm[k] = original local
 * vertex id at internal position k, spatially ordered. Layout metadata
 * only — results are identical with or without it. */
const int32_t *mv_graph_locality_hint(const mv_graph *g);

/* Windowed degree order: refine an internal order so that every SELL slice
 * (64 consecutive positions) holds vertices of nearly equal degree while a
 * vertex never leaves its window of `window` consecutive positions. Host
 * only, needs no GPU. hint[k] = local vertex at position k (NULL: the
 * identity), xadj has lnv+1 entries; out[lnv] receives the refined order.
 * window: a power of two >= 128; quant >= 1; group: a power of two with
 * 1 <= group <= window/64. For each aligned window of `window` positions:
 *  - its vertices are stable-sorted by key (degree + quant - 1) / quant,
 *    descending, and cut into rows of 64;
 *  - with R = window/64 rows and G = R/group, sorted row r goes to row
 *    position (r mod G)*group + r/G, so every aligned run of `group` rows
 *    samples the window's degree spectrum evenly (G == 1: plain sorted);
 *  - a short last window (lnv not a multiple of window, or window > lnv)
 *    keeps the plain sorted order.
 * Layout metadata only, like the hint. Returns non-zero, writing nothing,
 * for arguments outside the ranges above. */
int mv_degree_window_order(const int32_t *hint, const int64_t *xadj,
                           int64_t lnv, int64_t window, int64_t quant,
                           int64_t group, int32_t *out);

/* The integer arithmetic of the sweep's row schedule (mv_sweep_info states
 * the rules), as the engine computes it. Host only: needs no GPU and no
 * engine. Three answers in one call:
 *  - *default_unit: the queue unit U a graph of lnv vertices gets with no
 *    MV_SWEEP_UNIT on a sweep grid of sweep_grid blocks (0 = static);
 *  - *default_row_group: its row_group under the default degree window of
 *    `window` vertices (0 = the windowed order is off for this graph);
 *  - one queued launch over `positions` SELL positions in units of `unit`
 *    rows on launch_grid blocks: the return value is the number of ticket
 *    words in use, h (a power of two <= 8), and tickets[0..h) receive what
 *    the launch takes from each word — one ticket per unit in all.
 *    tickets has room for 8.
 * Returns -1, writing nothing, for lnv, window or positions < 0 or
 * sweep_grid, unit or launch_grid < 1. */
int mv_sweep_schedule(int64_t lnv, int sweep_grid, int64_t window,
                      int64_t positions, int unit, int launch_grid,
                      int *default_unit, int64_t *default_row_group,
                      int64_t *tickets);

/* ---- the hot path (replaces distLouvainMethod, dspl.hpp:1280-1441) ---- */

typedef struct mv_engine mv_engine;

#define MV_COMM_ID_BYTES 128
/* ncclGetUniqueId wrapper (rank 0 only; returns 0 on success). */
int mv_comm_id(void *id_128_bytes);

/* Create the engine on HIP device `device`. nranks > 1 requires the 128-byte
 * id from mv_comm_id on every rank. Aborts loudly (non-zero + message on
 * stderr) when no GPU or no RCCL — there is no CPU fallback. */
mv_engine *mv_engine_create(int device, int rank, int nranks,
                            const void *comm_id_or_null);
void mv_engine_destroy(mv_engine *e);

/* ---- loopback transport (hardware-validation harness) ----
 * Runs nranks engines in ONE process on ONE device, one host thread per
 * rank; the collectives become device-to-device copies + host barriers
 * while every kernel and every byte of the multi-rank protocol stays the
 * p>1 production path. Purpose: executing the partitioned engine on a
 * single-GPU box, where RCCL refuses two ranks on one device. The product
 * multi-GPU path (bench.py, mv355) always uses RCCL. */
typedef struct mv_lb_session mv_lb_session;
mv_lb_session *mv_lb_create(int nranks);
void mv_lb_destroy(mv_lb_session *s);
/* Like mv_engine_create but exchanges ride the loopback session. */
mv_engine *mv_engine_create_lb(int device, int rank, int nranks,
                               mv_lb_session *s);

/* Upload the per-rank CSR to HBM (device layout: DESIGN.md §data layout). */
int mv_engine_load_graph(mv_engine *e, const mv_graph *g);

/* Run Louvain phase 1 on the loaded graph: the drop-in for
 * distLouvainMethod(me, nprocs, dg, ..., lower, thresh, iters)
 * (dspl.hpp:1280-1284). Includes the exchangeVertexReqs setup
 * (dspl.hpp:1112-1272) like the reference's timed span. Returns prevMod
 * (the PREVIOUS iteration's modularity — dspl.hpp:1440); *iters_out gets
 * the iteration count. Collective: all ranks must call together. */
double mv_engine_run(mv_engine *e, double lower, double thresh,
                     int *iters_out);

/* Optional parity trace: before mv_engine_run, point the engine at caller
 * buffers receiving, per iteration k (1-based), this rank's targetComm
 * (dspl.hpp:404) at target_trace[(k-1)*lnv .. k*lnv) and the global
 * modularity at mod_trace[k-1]. cap bounds the recorded iterations.
 * Pass NULLs to disable. */
void mv_engine_set_trace(mv_engine *e, int64_t *target_trace,
                         double *mod_trace, int cap);

/* Perf counters for the last mv_engine_run (HIP-event timed, per stream). */
typedef struct {
    double total_ms;        /* whole run (setup + loop) */
    double sweep_ms;        /* K4 distExecuteLouvainIteration kernel time */
    int64_t sweep_launches;
    double halo_ms;         /* RCCL exchanges + pack/unpack */
    double setup_ms;        /* exchangeVertexReqs equivalent */
    int64_t edges_local;    /* directed edges on this rank */
    int iters;
} mv_stats;
void mv_engine_get_stats(const mv_engine *e, mv_stats *out);

/* Which K4 kernel shapes the last mv_engine_run launched, and the routing
 * state that chose them (tests assert on it; nothing here is timed).
 * The counters are host-side launch counts, zeroed where mv_stats is
 * (graph load and the start of a run); a launch over an empty range is not
 * issued and not counted. With the halo overlap on, the general and
 * iteration-1 kernels are launched twice per iteration (exports, then the
 * interior). The state fields are read from the engine when the call is
 * made: at nranks > 1 they describe the last run's setup (ghost discovery
 * and the SELL build happen inside the run), `overlap` after the
 * collective decision. */
typedef struct {
    int64_t general;          /* k4_sweep launches, all SLOTS together */
    int64_t general_slots[7]; /* ... by SLOTS = 4, 8, 12, 16, 24, 32, 48 */
    int64_t iter1_label_order;    /* k4_sweep_iter1, LBL_ASC = true */
    int64_t iter1_internal_order; /* k4_sweep_iter1, LBL_ASC = false */
    int64_t hi;               /* k4_sweep_hi launches */
    int64_t lh;               /* k4_sweep_lh launches */
    int64_t nhi, nlh;         /* degree-sorted positions [0,nhi) take the
                               * wave-per-vertex kernel, [nhi,nlh) the
                               * lane-hash kernel, [nlh,lnv) the others */
    int64_t nghost;           /* distinct remote tails of this rank */
    int64_t ssz;              /* export entries, summed over the peers */
    int64_t nexp;             /* exported vertices placed first (overlap) */
    int skewed;               /* max local degree > 256 */
    int overlap;              /* halo #1a overlapped in the last run */
    int rows_sorted;          /* input rows had ascending tails */
    int sell_sorted;          /* SELL rows re-sorted by internal index */
    int unit_weights;         /* every local edge weight == 1.0 */
    /* Windowed degree order (mv_degree_window_order), decided at graph
     * load. It applies only to a graph with a locality hint that is not
     * skewed. MV_DEG_WINDOW (vertices, a power of two >= 128; 0 = off) and
     * MV_DEG_QUANT (>= 1) are read at every load. A window set through
     * MV_DEG_WINDOW is honoured as given — a window longer than lnv is
     * reported as set and is one short window — with row_group =
     * min(window/64, 8). Without it the built-in default window applies
     * and row_group is the largest power of two <= min(window/64, rows per
     * wave), rows per wave = ceil(ceil(lnv/64) / waves of the full sweep
     * grid); below 2 the order is off for this graph. Off means
     * deg_window == 0, deg_quant == 1, row_group == 1. */
    int64_t deg_window;       /* effective window, vertices (0 = off) */
    int64_t deg_quant;        /* effective degree quantum */
    int64_t row_group;        /* rows of 64 positions a wave takes in turn
                               * in k4_sweep / k4_sweep_iter1 */
    int64_t sell_entries;     /* SELL image entries, padding included */
    /* Row queue of k4_sweep, decided at graph load. MV_SWEEP_UNIT (rows
     * per unit, 0 = off) and MV_SWEEP_GRID (caps the grid of k4_sweep and
     * k4_sweep_iter1, in blocks; the spill extents follow it; unset or 0 =
     * no cap) are read at every load. With sched_unit = U > 0 the rows of
     * a queued launch are cut into units of U rows; every wave starts with
     * the unit of its own index and takes the remaining ones from per-block-
     * group ticket words, one returning atomic add per unit plus one that
     * finds its queue dry, and the launch's grid is held to one resident
     * round (the occupancy query); row_group then only describes the
     * layout. Without MV_SWEEP_UNIT, U is the largest of 4 and 2 that
     * leaves every wave of the full grid two units or more, else 0;
     * a unit set through MV_SWEEP_UNIT is honoured as given. Either way
     * only the launches after the first-iterations slot variant queue
     * (MV_FIRST_ITERS), unless MV_SWEEP_QUEUE_FROM (read at load) names
     * another first iteration. k4_sweep_iter1, skewed graphs
     * (their spill extents are sized for the static schedule; they report
     * 0) and everything else keep the static row-group schedule. The
     * ticket words are zeroed at load and never reset: sched_tickets is
     * their sum when this call is made (with sched_unit > 0 the call waits
     * for the engine's stream and copies them; otherwise it touches no
     * device state), sched_tickets_expected the host's running total, over every
     * queued launch since the load, of one ticket per unit. The two are
     * equal exactly when every launch drained its queues and no wave
     * pulled past its first dry ticket. */
    int64_t sched_unit;       /* effective U (0 = static schedule) */
    int64_t sched_grid;       /* blocks of the last k4_sweep launch that ran
                               * to the end of the vertex range (the full
                               * range unless the halo overlap splits it) */
    int64_t sched_tickets;
    int64_t sched_tickets_expected;
    int64_t perm_identity;    /* 1: SELL position s holds internal vertex s
                               * (locality hint, not skewed, no exports-first
                               * partition), and the identity variants of
                               * k4_sweep / k4_sweep_iter1, which never read
                               * the permutation, are the ones launched */
    int64_t slot_bytes;       /* LDS bytes per slot and lane of the last
                               * k4_sweep launch of the run: 8 on a unit
                               * graph ({u32 key, u32 count}), 12 on a
                               * weighted one (u32 key + f64 sum); 0 if no
                               * k4_sweep ran. A launch counter like
                               * `general`. */
} mv_sweep_info;
void mv_engine_get_sweep_info(const mv_engine *e, mv_sweep_info *out);

/* What the halo of the last mv_engine_run put on the wire, per rank (tests
 * assert on it; nothing here is timed). Host-side counts, zeroed where
 * mv_sweep_info is (graph load and the start of a run) and taken where
 * the exchange plan is built, above the transport seam, so RCCL and
 * loopback report the same numbers. All zero at nranks == 1.
 * One "exchange" is one halo #1a label exchange: a run of K iterations
 * makes K of them without the overlap and K+1 with it (the pre-loop one
 * plus one per iteration, the last being the speculative one past the
 * exit); candidate discovery (prep_calls) follows every exchange.
 * The send_ / recv_ counters count (peer, exchange) pairs whose segment is
 * non-empty, by the arm the plan took: the whole segment, (index, label)
 * pairs of the changed entries, or nothing (no entry changed). The whole
 * segment goes when changed*12 >= segment*8. With MV_NO_DELTA every
 * non-empty segment is full. */
typedef struct {
    int64_t exchanges;
    int64_t send_full, send_compact, send_silent;
    int64_t recv_full, recv_compact, recv_silent;
    int64_t send_compact_entries; /* (index, label) pairs sent ... */
    int64_t recv_compact_entries; /* ... and received */
    int64_t prep_calls;           /* candidate discoveries */
    int64_t nrc_sum;  /* remote communities requested, summed over them */
    int64_t nrc_max;  /* ... the largest request of one discovery */
    int64_t nrc_zero; /* ... discoveries that requested none */
    int64_t nreq_sum; /* records the peers requested from this rank */
} mv_halo_info;
void mv_engine_get_halo_info(const mv_engine *e, mv_halo_info *out);

/* ---- beyond phase one: assignment, aggregation, multi-phase driver ----
 * The reference mini-app stops after one phase and never hands the
 * assignment out (main.cpp:164-196 prints modularity and iterations only);
 * unless noted, the entries below have no counterpart there. Definitions:
 * DESIGN.md, multi-phase section. */

/* This rank's lnv community labels (global vertex ids, original local
 * order) of the last mv_engine_run: the phase assignment. With K the
 * iteration the run exited at, that is currComm of iteration K-1
 * (dspl.hpp:1417-1422's pastComm at exit) — the last assignment that
 * passed the convergence test — or currComm of iteration K when K <= 2,
 * where pastComm is still the identity. In trace rows (0-based): K-3 for
 * K >= 3, row 0 for K == 2, the identity for K == 1. Works at any nranks;
 * costs nothing unless called. Returns non-zero before the first run. */
int mv_engine_get_communities(mv_engine *e, int64_t *out);

/* Aggregate g (single-rank) by comm[lnv] (labels in [0,nv)) on HIP device
 * `device`: labels are renumbered dense in ascending order into
 * map_out[lnv], and every directed fine edge (u, v, w) adds w to the
 * coarse edge (map[u], map[v]), map[u] == map[v] included (a coarse
 * self-loop). The result is a CSR with one entry per distinct pair, tails
 * ascending per row; weights are summed in a fixed order, so two calls
 * agree bit for bit. Returns NULL with a message on stderr for a label out
 * of range, a multi-rank graph, or no GPU. No reference counterpart. */
mv_graph *mv_coarsen_csr(int device, const mv_graph *g,
                         const int64_t *comm, int64_t *map_out);

/* Multi-phase Louvain (single rank). Level 0 is g; each phase loads the
 * current level, runs mv_engine_run(lower, thresh), takes the phase
 * assignment and — unless it merges nothing — aggregates it into a
 * proposed next level. A proposal whose q is below the current level's is
 * dropped and ends the run; a kept one ends it when it gains less than
 * thresh. q of a level = sum_c selfloop_c / W - sum_c deg_c^2 / W^2 on
 * that level's graph: the modularity of the partition of g the level
 * represents (the per-phase value mv_engine_run returns is the reference's
 * hybrid, dspl.hpp:407-456 after :458-471, and is reported separately).
 * max_phases < 1 means no cap but the safety bound of 64 phases.
 * The driver loads g itself and LEAVES THE ENGINE HOLDING THE LAST GRAPH
 * IT LOADED (a device copy of the last level, or of g): call
 * mv_engine_load_graph again before a plain mv_engine_run. Returns NULL
 * with a message on stderr, before any communication, when nranks > 1
 * (mv_engine_run_multiphase_dist below is the driver for that). */
typedef struct mv_hierarchy mv_hierarchy;
typedef struct { int iters; double run_mod; int64_t nv_in, ne_in;
                 double run_ms, coarsen_ms; int kept; } mv_phase_info;

mv_hierarchy *mv_engine_run_multiphase(mv_engine *e, const mv_graph *g,
                                       double lower, double thresh,
                                       int max_phases);
int  mv_hierarchy_phases(const mv_hierarchy *h);   /* phases run, >= 1 */
int  mv_hierarchy_levels(const mv_hierarchy *h);   /* kept coarse levels L */
/* Level 1..L (owned by the hierarchy); NULL outside that range. */
const mv_graph *mv_hierarchy_graph(const mv_hierarchy *h, int level);
/* Dense map level-1 -> level, for level 1..L; NULL outside. */
const int64_t *mv_hierarchy_map(const mv_hierarchy *h, int level);
/* q of level 0..L (level 0: g as singletons); NaN outside. */
double mv_hierarchy_modularity(const mv_hierarchy *h, int level);
/* Phase 1..phases: iterations and returned modularity of its run, size of
 * its input level, wall time of the run and of the aggregation (device
 * pipeline + the copy to the host level), and whether its proposal was
 * kept. Non-zero outside the range. */
int  mv_hierarchy_phase_info(const mv_hierarchy *h, int phase,
                             mv_phase_info *out);
/* What phase 1..phases proposed, kept or dropped: its community count and
 * the q of its coarse graph (nv_in and the current q when it merged
 * nothing). */
int  mv_hierarchy_phase_proposal(const mv_hierarchy *h, int phase,
                                 int64_t *nv_out, double *q_out);
/* Final community of each vertex of g: the composed kept maps, dense ids
 * in [0, nv of level L) (the identity when L == 0). */
const int64_t *mv_hierarchy_communities(const mv_hierarchy *h);
void mv_hierarchy_free(mv_hierarchy *h);

/* ---- the same two steps across ranks ----
 * The coarse graph of a partitioned level is the coarse graph of the
 * stitched level (dense ids in ascending global label order, one entry per
 * distinct pair, tails ascending), split evenly: coarse vertex c belongs to
 * rank r with parts'[r] = (nc * r) / nranks <= c < parts'[r + 1]. A rank
 * may own no vertices (nc < nranks); such a slice loads and runs like any
 * other. A coarse weight is the sum, in ascending rank order, of the
 * per-rank partial sums, each taken in the rank's local edge order with
 * the fixed-order reduction of mv_coarsen_csr (a pair with partials from
 * more than 32 ranks is summed by that reduction's fixed tree over the
 * rank-ordered partials instead of left to right): no floating-point atomics,
 * bit-identical run to run, exact for integer-valued weights, and at
 * nranks == 1 bit-identical to mv_coarsen_csr. */

/* Collective. Aggregate the partitioned graph (this rank's slice g) by
 * comm[lnv] (global labels in [0,nv)). Returns this rank's slice of the
 * coarse graph (parts = the even split above); map_out[lnv] receives the
 * global dense coarse id of each local vertex. NULL on EVERY rank if any
 * rank saw an error (a label out of range, a graph that is not this rank's
 * slice, nv >= 2^31, or 2^31 - 1 or more local edges or received partial
 * edges on some rank). Needs no mv_engine_run and leaves the loaded graph
 * alone. */
mv_graph *mv_engine_coarsen_dist(mv_engine *e, const mv_graph *g,
                                 const int64_t *comm, int64_t *map_out);

/* Collective. The multi-phase driver at any nranks (nranks == 1 included,
 * where it equals mv_engine_run_multiphase bit for bit). The driver rule
 * is unchanged; "merges nothing" means global nc == global nv, and q of a
 * level is reduced from per-rank (selfloops, deg^2, W) in rank order, so
 * every rank takes the same keep / drop / stop decision. The engine is
 * left holding the last level it loaded. The mv_hierarchy_* accessors
 * take a per-rank meaning:
 *  - mv_hierarchy_graph(h, k) is this rank's slice of level k; its parts
 *    say who owns what;
 *  - mv_hierarchy_map(h, k) has one entry per vertex of this rank's slice
 *    of level k-1 (of g for k = 1), values are global ids of level k;
 *  - mv_hierarchy_communities(h) has one final global dense id per local
 *    vertex of g (the vertex's own global id when no level was kept);
 *  - mv_hierarchy_modularity, _phases, _levels, _phase_info (nv_in and
 *    ne_in are global counts) and _phase_proposal return the same values
 *    on every rank (wall times excepted). */
mv_hierarchy *mv_engine_run_multiphase_dist(mv_engine *e, const mv_graph *g,
                                            double lower, double thresh,
                                            int max_phases);

#ifdef __cplusplus
}
#endif

#endif /* MINIVITE_HIP_H */
