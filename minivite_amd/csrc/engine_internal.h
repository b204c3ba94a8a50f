// engine_internal.h — what the engine's translation units share. Not part
// of the C-ABI (that is include/minivite_hip.h).
//
//   engine.hip      lifecycle, graph load + SELL build, the support kernels
//                   K1-K10, the transport seam (RCCL / loopback), the halo,
//                   and mv_engine_run: the phase-one loop
//   sweep.hip       the K4 sweep kernels and their launch dispatch (sweep_*)
//   multiphase.hip  the distributed aggregation over the transport seam and
//                   the one multi-phase driver (mv_hierarchy)
//   coarsen.hip     the transport-free aggregation kernels (coarsen.h);
//                   includes neither this header nor RCCL
// device_util.h   what all four share: HIP_CHECK, DevBuf / PinBuf (the one
//                 owner of device and pinned memory), the device binary
//                 search, ceil_log2, read_back, the iota and bounds kernels
// cub_util.h      the hipCUB wrappers (engine.hip and coarsen.hip)
// sweep_schedule.h holds the schedule's host arithmetic (no HIP).
#ifndef MINIVITE_ENGINE_INTERNAL_H
#define MINIVITE_ENGINE_INTERNAL_H

#include <condition_variable>
#include <mutex>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/minivite_hip.h"
#include "device_util.h"
#include "sweep_schedule.h"

#define NCCL_CHECK(x)                                                         \
    do {                                                                      \
        ncclResult_t _e = (x);                                                \
        if (_e != ncclSuccess) {                                              \
            std::fprintf(stderr, "RCCL error %s at %s:%d: %s\n",              \
                         ncclGetErrorString(_e), __FILE__, __LINE__, #x);     \
            std::abort();                                                     \
        }                                                                     \
    } while (0)

struct Cinfo {     // localCinfo / localCupdate entry (Comm, dspl.hpp:61-66)
    i64 size;
    double degree;
};

struct Info16 {    // wire record for cinfo replies / delta routing: the
    i64 size;      // CommInfo payload (dspl.hpp:68-72) minus the community
    double degree; // id, which both ends know by position
};

// Speculation-safe index clamp: semantically-exclusive branches may be
// if-converted into two unconditional loads + a value select, so the
// un-taken side's address must still be dereferenceable (ghost/rc
// buffers are never null — load_graph keeps 1-element dummies — and
// indices are clamped non-negative).
__device__ __forceinline__ i64 clamp0(i64 x) { return x > 0 ? x : 0; }

__device__ __forceinline__ i64 dev_bsearch(const i64 *a, i64 n, i64 key) {
    i64 p = dev_lower_bound(a, n, key);
    return (p < n && a[p] == key) ? p : -1;
}

// one point-to-point message of a batched exchange (see exchange())
struct Xfer {
    int peer;
    void *ptr;
    ncclDataType_t ty;
    i64 count; // elements of ty
};

constexpr int QUEUE_HEAD_STRIDE = 16; // u64 between the ticket words: a
                                      // 128-B line each

// ------------------------------------------------------------------------
// Loopback transport: nranks engines in one process on one device, one
// host thread per rank (see the header note in minivite_hip.h). Exchange
// payloads move by device-to-device hipMemcpyAsync between the engines'
// buffers; host barriers stand in for the collective rendezvous. All
// reductions run in rank order (deterministic, like the RCCL fixed-tree
// at these tiny sizes and like the oracle).
struct mv_lb_session {
    int nranks;
    std::mutex mu;
    std::condition_variable cv;
    int count = 0;
    uint64_t gen = 0;
    struct Post {
        const std::vector<Xfer> *sends = nullptr; // exchange(): my send list
        const double *red = nullptr;
        std::vector<int64_t> cnts;
    };
    std::vector<Post> posts;
    explicit mv_lb_session(int n) : nranks(n), posts(n) {}
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t g = gen;
        if (++count == nranks) {
            count = 0;
            gen++;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
    }
};

// Everything load_graph / run derive from ONE graph: the device image, the
// per-run halo state and the logical sizes that go with them. A reload
// replaces the whole value (free_graph_state), so a member added here needs
// no separate reset.
struct mv_graph_state {
    int overlap = 0;               // this run overlaps #1a (p>1, !skewed)
    i64 nexp = 0;                  // SELL positions [0,nexp) = exported

    // graph (device)
    i64 nv = 0, lnv = 0, lne = 0, base = 0, bound = 0;
    int sort_bits = 64; // ceil_log2(nv): radix sort width for id keys
    std::vector<i64> parts_h;
    DevBuf<i64> d_parts;
    DevBuf<i64> d_xadj;
    DevBuf<i64> d_tails;   // raw global tails (kept for setup)
    DevBuf<double> d_ew;   // edge weights (CSR order)
    int unit_weights = 1;
    int rows_sorted = 1; // per-row tails ascending (reference CSR order)
    int sell_sorted = 0; // SELL rows re-sorted by internal index (unit)
    int perm_identity = 0; // d_perm[s] == s: build_sell's iota, unpermuted
    i64 max_degree = 0;

    // internal layout
    DevBuf<unsigned> d_sigma;     // internal -> original local id
    DevBuf<unsigned> d_sigma_inv; // original local id -> internal
    int has_hint = 0;
    // windowed degree order folded into sigma at load (0 / 1 / 1 = off) and
    // the row-group length the lane-per-vertex sweeps run with
    i64 deg_window = 0, deg_quant = 1;
    int row_group = 1;
    i64 sell_entries = 0; // SELL image size, padding included

    // SELL-64 image (built in the per-run setup span)
    DevBuf<unsigned> d_deg;          // degree per INTERNAL index
    DevBuf<unsigned> d_iota, d_perm; // SELL pos -> internal
    DevBuf<i64> d_chunk_off;         // nchunks+1 element offsets
    i64 nchunks = 0;
    DevBuf<int> d_sell_tidx;
    DevBuf<double> d_sell_w; // weighted graphs only

    // per-run state (device)
    DevBuf<i64> d_curr, d_past, d_target;
    DevBuf<double> d_vdeg, d_cw;
    DevBuf<Cinfo> d_cinfo, d_cupd;
    DevBuf<double> d_partials; // 2 * nblocks
    PinBuf<double> h_partials; // pinned mirror (pageable D2H costs
                               // ~40 us/iteration in staging latency)
    DevBuf<double> d_red;      // 2 doubles for allreduce

    // ghosts / halo
    DevBuf<i64> d_ghosts; // sorted unique remote tails
    i64 nghost = 0;
    // u32 community views (multi-rank sweeps; rebuilt per iteration from
    // the persistent LABEL arrays once rc_ids is known)
    DevBuf<unsigned> d_vcurr;   // lnv
    DevBuf<unsigned> d_vghost;  // nghost
    DevBuf<unsigned> d_vtarget; // lnv (persisted back as labels)
    DevBuf<i64> d_svdata; // vertices peers want from me (global ids)
    DevBuf<unsigned> d_svdata_int;
    i64 ssz = 0;
    std::vector<i64> send_off, recv_off; // per-peer offsets into svdata / ghosts
    DevBuf<i64> d_scdata;                // packed comms to export

    // halo #1a delta compaction (send side tracks the last label sent per
    // export; receive side keeps the persistent ghost label image)
    int use_delta = 0;
    DevBuf<i64> d_last_sent;           // ssz, init -1 (all changed)
    DevBuf<unsigned> d_chg_idx;        // ssz, segment-based layout
    DevBuf<i64> d_chg_lab;             // ssz
    DevBuf<unsigned long long> d_chg_cnt; // nranks counters
    DevBuf<i64> d_cntmat;              // nranks*nranks image, every count
                                       // allgather (allgather_counts)
    PinBuf<i64> h_cntmat;              // pinned mirror (delta counts)
    DevBuf<i64> d_soff;                // send_off on device (nranks+1)
    DevBuf<i64> d_ghost_labels;        // nghost persistent labels
    DevBuf<unsigned> d_rchg_idx;       // nghost recv compact indices
    DevBuf<i64> d_rchg_lab;            // nghost recv compact labels

    // remote community info (per iteration)
    DevBuf<i64> d_cand, d_cand_sorted;
    DevBuf<i64> d_rc_ids;
    DevBuf<Info16> d_rc_info; // aligned with rc_ids
    DevBuf<Info16> d_rcu;     // remoteCupdate accumulators
    DevBuf<i64> d_req_ids;    // ids other ranks requested from me
    DevBuf<Info16> d_req_info;
    DevBuf<i64> d_bounds;     // nranks+1
    DevBuf<unsigned long long> d_count;
    DevBuf<char> d_cub_tmp; // bytes

    // spill for K4 (per-thread extents; uniform for flat degree
    // distributions, degree-prefix-sized for skewed ones)
    DevBuf<i64> d_spill_k;
    DevBuf<double> d_spill_a;
    DevBuf<i64> d_spill_off;
    int skewed = 0;
    int sweep_grid = 0;

    // row queue of the lane-per-vertex sweeps (RowQueue): rows per unit
    // (0 = static schedule), the ticket word (zeroed at load, never reset)
    // and the host's running total of tickets its launches must consume
    int sched_unit = 0;
    int sched_from = 0; // first iteration whose k4_sweep launches queue
                        // (MV_SWEEP_QUEUE_FROM; 0 = after the first-
                        // iterations slot variant)
    int sched_grid = 0; // blocks of the last k4_sweep launch that ran to lnv
    DevBuf<unsigned long long> d_ticket; // QUEUE_HEADS strided words
    unsigned long long tickets_total[QUEUE_HEADS] = {};

    // hash-aggregation bands over the degree-sorted positions:
    // [0, nhi) = wave-per-vertex hubs (unit only), [nhi, nlh) = lane-hash
    // band, [nlh, lnv) = LDS slots + linear spill
    i64 nhi = 0;
    i64 nlh = 0;
    DevBuf<unsigned> d_lh_list; // compact candidate lists (hash/2)
    DevBuf<int> d_tidx32;   // lne pre-translated tails (hub kernels)
    DevBuf<i64> d_hash_off; // nlh+1 slot offsets (per-vertex caps are powers of two)
    DevBuf<i64> d_hkeys;
    DevBuf<double> d_hacc;
    i64 hash_total = 0;     // slots in use (the per-iteration key reset)
    i64 hash_hub_elems = 0; // prefix the wave kernel atomics into (needs
                            // zeroed accumulators each iteration)

    // phase assignment of the last run (mv_engine_get_communities): the
    // rotated buffer that holds it — past at exit, or curr when past is
    // still the identity (K <= 2) — converted to labels only on request
    const i64 *res_src = nullptr;
    DevBuf<i64> d_res; // lnv labels, original local order

    // trace
    i64 *trace_target = nullptr;
    double *trace_mod = nullptr;
    int trace_cap = 0;
    DevBuf<i64> d_trace_tmp;
};

struct mv_engine : mv_graph_state {
    int device = 0, rank = 0, nranks = 1;
    int num_cus = 1; // compute units of the device
    // resident blocks per CU of this engine's k4_sweep instantiations, by
    // [SLOTS index][UNIT][IDP] (the occupancy query; 0 = not asked yet)
    int sweep_per_cu[7][2][2] = {};
    ncclComm_t comm = nullptr;
    ncclComm_t comm2 = nullptr; // halo #1a's communicator (overlap mode)
    mv_lb_session *lb = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // halo #1a rides here, overlapped
    hipEvent_t ev_p1 = nullptr;    // sweep part 1 (exports) done [stream]
    hipEvent_t ev_p2 = nullptr;    // full sweep + writeback done [stream]
    hipEvent_t ev_cinfo = nullptr; // K6 + delta application done [stream]
    hipEvent_t ev_halo = nullptr;  // next-iteration pipeline done [stream2]

    mv_stats stats{};
    mv_sweep_info sweep{}; // launch counters only; state is read on request
    mv_halo_info halo{};   // what the halo plans of the last run carried
    std::vector<hipEvent_t> ev_pool;
    int ev_used = 0;

    hipEvent_t ev_pair() {
        if (ev_used >= (int)ev_pool.size()) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
        return ev_pool[ev_used++];
    }
};

// ---- engine.hip: the transport seam, and what else multiphase.hip needs
void exchange(mv_engine *e, const std::vector<Xfer> &sends,
              const std::vector<Xfer> &recvs, ncclComm_t comm,
              hipStream_t stream);
void alltoallv(mv_engine *e, const void *send, const i64 *soff, void *recv,
               const i64 *roff, size_t elem_bytes, ncclDataType_t ty,
               ncclComm_t comm, hipStream_t stream);
void allgather_counts(mv_engine *e, const i64 *mine, bool on_device,
                      i64 *matrix, ncclComm_t comm, hipStream_t stream);
void comm_allreduce_host(mv_engine *e, double *vals, int n);
// The last run's phase assignment as LABELS in original local order, in
// e->d_res (device). Null before the first run.
const i64 *phase_labels_device(mv_engine *e);
// The values of d_vals[0,n) outside [base, bound), sorted and distinct, in
// d_ids (grown to fit, never null); returns their count. The values are
// ids below 2^bits. Synchronises st.
i64 remote_ids(hipStream_t st, i64 n, const i64 *d_vals, i64 base, i64 bound,
               int bits, DevBuf<i64> &d_ids);
// off[r+1] - off[r] = what rank r sends to `me`: column `me` of a count
// matrix (allgather_counts). My own entry counts only where my segment
// travels with the others.
inline void recv_offsets(const std::vector<i64> &matrix, int p, int me,
                         bool with_own, std::vector<i64> &off) {
    off.assign(p + 1, 0);
    for (int r = 0; r < p; r++)
        off[r + 1] = off[r] + (r == me && !with_own
                                   ? 0
                                   : matrix[(size_t)r * p + me]);
}

// ---- sweep.hip: the K4 launches of mv_engine_run ----
enum SweepIter1 { // the kernel of iteration 1
    ITER1_GENERAL,  // k4_sweep, like every later iteration
    ITER1_INTERNAL, // k4_sweep_iter1: unit, rows in internal order
    ITER1_UNIT,     // ... unit, rows label-ascending
    ITER1_WEIGHTED, // ... weighted, rows label-ascending
};
// what the sweep launches of one run share, built once before the loop
struct SweepPlan {
    double constant;     // 1 / total edge weight (dspl.hpp:129)
    int slots_first = 8; // k4_sweep's LDS slots per lane in iterations
    int first_iters = 0; // 1..first_iters,
    int slots_rest = 8;  // and after them
    int queue_from = 0;  // first iteration that queues k4_sweep rows (0: none)
    SweepIter1 iter1 = ITER1_GENERAL;
};
SweepPlan sweep_plan(const mv_engine *e, double constant);
// An iteration's sweep. d_curr / d_target are the rotated community arrays:
// the view itself at one rank; at p > 1 e->d_vcurr / e->d_vtarget are swept.
// The hash-aggregation bands [0, nlh) of a skewed graph: k4_sweep_hi / _lh.
void sweep_hash_bands(mv_engine *e, const SweepPlan &plan, int iter,
                      const i64 *d_curr, i64 *d_target);
// SELL positions [s0, s1): k4_sweep, or k4_sweep_iter1 at iteration 1.
void sweep_positions(mv_engine *e, const SweepPlan &plan, int iter,
                     const i64 *d_curr, i64 *d_target, i64 s0, i64 s1);

#endif
