// sweep.hip — K4, the Louvain sweep: its four kernel shapes and the launch
// dispatch mv_engine_run drives them through (engine_internal.h: sweep_*).
// Built with -ffp-contract=off: the FP discipline note in engine.hip.

#include <type_traits>

#include "engine_internal.h"

namespace {

// ---- K4: THE sweep (distExecuteLouvainIteration, dspl.hpp:276-405) ----
// One lane per vertex over the SELL image (see the layout note at the top).
// The clmap/counter hash (dspl.hpp:230-274) lives as per-lane slot arrays:
// the first SLOTS distinct neighbor communities in LDS (lane-strided,
// conflict-free for ds b64), the tail in a per-thread global spill region
// (only populated while communities are still fine-grained; L2-resident).
// The current community's accumulator is a register (the reference's
// counter[0], dspl.hpp:312-318).
//
// Community encoding. Every sweep runs over a u32 VIEW (see k_build_view):
// a value < lnv is a local internal slot (cinfo/cupd index), a value >= lnv
// is lnv + rc index (rc_info/rcu index). Equality probes only need
// community identity and the info lookups need exactly this index, so the
// per-edge community gather (the sweep's dominant random traffic) is 4 B
// with NO added indirection on the info lookups. Only the reference's
// tie-break and singleton guard need label ORDER (dspl.hpp:214-225), and
// only per DISTINCT candidate: labels come from sigma (+base) or rc_ids,
// fetched lazily — only when a gain tie actually needs the order — so the
// common strict-greater path costs no label traffic at all (dspl.hpp:
// 174-228 order semantics preserved bit-for-bit). (A pure-label variant
// was measured and rejected: sigma_inv[label]->cinfo adds a dependent-load
// chain to the latency-bound gain scan — 4M 104G vs 110G handles vs this
// design.)
//
// Mode (template parameter MR). MR=true is the multi-rank VIEW mode above.
// MR=false is single-rank SLOT mode: the view without ghosts. At one rank
// every community is local and base is 0, so the persistent u32 slot
// arrays ARE the view, a label is sigma[slot] (u32), and every remote
// branch folds away at compile time — the ghost/rc pointers are passed
// (1-element dummies) but never read.
//
// Shapes: k4_sweep (the general LDS-slot sweep), k4_sweep_iter1 (streaming
// first iteration), k4_sweep_hi (wave-per-vertex hubs) and k4_sweep_lh
// (lane-hash band; view form at every rank count). They share the
// fragments below, each written once.

// label type: i64 global ids in view mode, the u32 sigma value in slot mode
template <bool MR> using label_t = std::conditional_t<MR, i64, unsigned>;

// label of an owned internal slot
template <bool MR>
__device__ __forceinline__ label_t<MR> own_label(i64 v, i64 base,
                                                 const unsigned *sigma) {
    if constexpr (MR) return base + (i64)sigma[v];
    else return sigma[v];
}

// label of a view value (tie-break / singleton-guard order only,
// dspl.hpp:214-225). clamp0: the un-taken rc_ids side must stay
// dereferenceable when the select is if-converted (see clamp0).
template <bool MR>
__device__ __forceinline__ label_t<MR> label_of(unsigned v, i64 lnv, i64 base,
                                                const unsigned *sigma,
                                                const i64 *rc_ids) {
    if constexpr (MR)
        return (v < lnv) ? own_label<MR>(v, base, sigma)
                         : rc_ids[clamp0(v - lnv)];
    else return sigma[v];
}

// community {size, degree}: localCinfo, or the fetched remote record
// (dspl.hpp:296-307)
template <bool MR>
__device__ __forceinline__ Cinfo comm_info(unsigned v, i64 lnv,
                                           const Cinfo *cinfo,
                                           const Info16 *rc_info) {
    if (!MR || v < lnv) return cinfo[v];
    const Info16 c = rc_info[v - lnv];
    return {c.size, c.degree};
}

// one side of a move: (dsize, ddeg) onto localCupdate / remoteCupdate
template <bool MR>
__device__ __forceinline__ void comm_add(unsigned c, i64 dsize, double ddeg,
                                         i64 lnv, Cinfo *cupd, Info16 *rcu) {
    if (!MR || c < lnv) {
        Cinfo *u = &cupd[c];
        atomicAdd(&u->degree, ddeg);
        atomic_add_i64(&u->size, dsize);
    } else {
        Info16 *u = &rcu[c - lnv];
        atomicAdd(&u->degree, ddeg);
        atomic_add_i64(&u->size, dsize);
    }
}

// the 4-case move update (dspl.hpp:331-399); SRC_MR / DST_MR: whether that
// side can be remote (at iteration 1 the source is always local)
template <bool SRC_MR, bool DST_MR>
__device__ __forceinline__ void move_update(unsigned from, unsigned to,
                                            double vdeg, i64 lnv, Cinfo *cupd,
                                            Info16 *rcu) {
    comm_add<SRC_MR>(from, -1, -vdeg, lnv, cupd, rcu);
    comm_add<DST_MR>(to, 1, vdeg, lnv, cupd, rcu);
}

// Edges go in chunks of CH: issue the CH independent tail loads and the CH
// dependent gathers together (the per-edge serial load->gather->probe chain
// was the measured bound: 80% SQ_WAIT_ANY with LDS and VALU idle), then
// consume sequentially in edge order (bit-exact -w accumulation,
// dspl.hpp:240-271). Steps past the row end re-load the row's first slot.
constexpr int CH = 8;

template <bool UNIT, typename T>
__device__ __forceinline__ void load_tails(i64 ebase, int k0, int m,
                                           const int *sell_tidx,
                                           const double *sell_w,
                                           T (&tb)[CH], double (&wb)[CH]) {
#pragma unroll
    for (int j = 0; j < CH; j++) {
        const i64 slot = (j < m) ? ebase + (i64)(k0 + j) * 64 : ebase;
        tb[j] = sell_tidx[slot];
        if (!UNIT) wb[j] = sell_w[slot];
    }
}

// the communities of a chunk's tails
template <bool MR, typename T>
__device__ __forceinline__ void gather_comms(const T (&tb)[CH], i64 lnv,
                                             const unsigned *vcurr,
                                             const unsigned *vghost,
                                             unsigned (&cb)[CH]) {
#pragma unroll
    for (int j = 0; j < CH; j++)
        cb[j] = (!MR || tb[j] < lnv) ? vcurr[tb[j]]
                                     : vghost[clamp0(tb[j] - lnv)];
}

// tails (+ weights unless UNIT) and their communities
template <bool MR, bool UNIT>
__device__ __forceinline__ void load_chunk(i64 ebase, int k0, int m, i64 lnv,
                                           const int *sell_tidx,
                                           const double *sell_w,
                                           const unsigned *vcurr,
                                           const unsigned *vghost,
                                           i64 (&tb)[CH], double (&wb)[CH],
                                           unsigned (&cb)[CH]) {
    load_tails<UNIT>(ebase, k0, m, sell_tidx, sell_w, tb, wb);
    gather_comms<MR>(tb, lnv, vcurr, vghost, cb);
}

// dQ gain (dspl.hpp:212) — operand order and parenthesisation are the
// reference's; with -ffp-contract=off this carries its exact bits
__device__ __forceinline__ double dq_gain(double eiy, double eix, double vdeg,
                                          double ay, double ax,
                                          double constant) {
    return 2.0 * (eiy - eix) - 2.0 * vdeg * (ay - ax) * constant;
}

// first probe position in a power-of-two open-addressed region (Fibonacci)
__device__ __forceinline__ i64 hash_start(unsigned tcomm, i64 cap) {
    return (i64)(((uint64_t)tcomm * 0x9E3779B97F4A7C15ull) >> 32) & (cap - 1);
}

// distGetMaxIndex, lane form (dspl.hpp:174-228), one candidate (y, eiy):
// strict-greater gain, gain ties to the smaller label (:214-215). With the
// label tie-break the argmax is a total order, so any scan order gives the
// reference's answer. The scan loop stays in the calling kernel (as one
// helper with a candidate functor it cost the view-mode sweep an
// occupancy step: 74 VGPRs instead of 72).
template <bool MR>
__device__ __forceinline__ void argmax_step(
    unsigned y, double eiy, double eix, double vdeg, double ax,
    double constant, i64 lnv, i64 base, const unsigned *sigma,
    const Cinfo *cinfo, const i64 *rc_ids, const Info16 *rc_info,
    double &maxGain, unsigned &maxIndex, i64 &maxSize) {
    const Cinfo c = comm_info<MR>(y, lnv, cinfo, rc_info);
    const double curGain = dq_gain(eiy, eix, vdeg, c.degree, ax, constant);
    if (curGain > maxGain) {
        maxGain = curGain;
        maxIndex = y;
        maxSize = c.size;
    } else if (curGain == maxGain && curGain != 0.0) {
        // real branch, not a select: the label loads must not be folded
        // into the gain-compare dataflow (ROCm 7.2 if-conversion
        // miscompile)
        if (label_of<MR>(y, lnv, base, sigma, rc_ids) <
            label_of<MR>(maxIndex, lnv, base, sigma, rc_ids)) {
            maxIndex = y;
            maxSize = c.size;
        }
    }
}

// ... and the singleton guard that closes the scan (dspl.hpp:224-225)
template <bool MR>
__device__ __forceinline__ unsigned singleton_guard(
    unsigned maxIndex, i64 maxSize, unsigned cc, i64 ccSize, i64 lnv,
    i64 base, const unsigned *sigma, const i64 *rc_ids) {
    if (maxSize == 1 && ccSize == 1 && maxIndex != cc) {
        if (label_of<MR>(maxIndex, lnv, base, sigma, rc_ids) >
            label_of<MR>(cc, lnv, base, sigma, rc_ids))
            maxIndex = cc;
    }
    return maxIndex;
}

// distGetMaxIndex, wave form: each lane holds its best candidate as (gain
// bg, packed bl = label << 32 | view, community size bs); reduce to lane 0
// under the total order (gain desc, bl asc) — label order decides and the
// view rides along for free; order-independent, so the reduce tree
// reproduces dspl.hpp:214-215 exactly. A lane without a positive-gain
// candidate holds the neutral element (0.0, INT64_MAX) and can never win.
__device__ __forceinline__ void wave_reduce_best(double &bg, i64 &bl,
                                                 i64 &bs) {
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_down(bg, off, 64);
        const i64 ol = __shfl_down(bl, off, 64);
        const i64 os = __shfl_down(bs, off, 64);
        if (og > bg || (og == bg && ol < bl)) {
            bg = og;
            bl = ol;
            bs = os;
        }
    }
}

// Row schedule of the lane-per-vertex sweeps (k4_sweep, k4_sweep_iter1).
// Row r of a launch is positions s_begin + 64r .. + 63, one per lane. The
// rows are cut into consecutive units of U rows, unit k = rows [kU,
// min((k+1)U, rows)); a wave walks the rows of a unit in order and then
// gets its next unit in one of two ways. Everything but the lane's
// position is wave-uniform (SGPRs).
//
// Static (RowQueue::ticket == nullptr): U is the row group S and wave x
// takes units x, x + waves, x + 2*waves, ... With the windowed degree
// order every wave then walks whole groups of S rows, each a sample of its
// window's degree spectrum, instead of the same degree rank of every
// window (a grid stride of 8192 waves is a multiple of every window
// length). S == 1 is the plain grid stride.
//
// Queue (ticket != nullptr; non-skewed graphs only, see choose_row_queue).
// Wave x still starts with unit x, but then takes units instead of owning a
// fixed set. The units from `waves` on are dealt round-robin onto `heads`
// ticket words, a word per group of blocks (block & (heads - 1): with the
// round-robin block dispatch that is one word per XCD, but nothing depends
// on it). Lane 0 does one returning device-scope atomicAdd on its block's
// word, readfirstlane broadcasts it, and ticket i of head h is queued unit
// i * heads + h. A wave stops at its first unit past the end, so a launch
// over nu units consumes exactly nu tickets whatever the residency or the
// arrival order — its queued units plus one dry ticket for each wave that
// had a first unit — and each head a share the host knows in advance. No
// barrier, no spin: a wave that starts late finds fewer units, and waves
// that finish light units early take more of them. The words are never
// reset; the host passes each launch the running totals as bases (launches
// of one engine are serial on one stream). A launch takes far fewer than
// 2^32 tickets, so the low words' difference is enough. Any thread may
// then run any vertex, which is why the spill extents must be uniform
// (k_spill_uniform) for this mode.
// Why this shape (measured at n=2^22, experiments/RESULTS.md): one word
// saturates near 88 returning adds/us, and a 0.24 ms launch with a ticket
// per unit AND per first unit needs 130/us at U=2; even the one dry ticket
// per wave, all landing as a round of waves ends, holds SIMD slots for
// tens of microseconds on one word. Eight words and a ticket-free first
// unit bring the queue's cost under what the even finish gains.
struct RowQueue {
    unsigned long long *ticket; // device words, monotonic; null = static
    unsigned base[QUEUE_HEADS]; // low word of each at launch start
    int unit;                   // rows per unit (static: the row group S)
    int heads;                  // words in use: a power of two <= blocks
};
struct RowWalk {
    int row;     // the current row of the launch
    int row_end; // one past the current unit's last row
    unsigned k;  // static: the current unit
};
// enter unit k of `unit` rows; returns the lane's first position, or s_end
// past the end
__device__ __forceinline__ i64 unit_enter(unsigned k, i64 s_begin, i64 s_end,
                                          int unit, RowWalk &w) {
    const i64 rows = (s_end - s_begin + 63) >> 6;
    const i64 row = (i64)k * unit;
    if (row >= rows) return s_end;
    w.k = k;
    w.row = (int)row;
    w.row_end = (int)(row + unit < rows ? row + unit : rows);
    return s_begin + row * 64 + (threadIdx.x & 63);
}
// Every lane-per-vertex launch has 256-thread blocks (__launch_bounds__ and
// the launch sites), so the walk takes the block size as a constant: read
// from the dispatch packet it is a vector load, and its wait at a unit end
// also drains the row's stores and atomics (they count in vmcnt on gfx950).
constexpr int SWEEP_BLOCK = 256;
__device__ __forceinline__ unsigned sweep_waves() {
    return gridDim.x * (SWEEP_BLOCK >> 6);
}
__device__ __forceinline__ i64 row_first(i64 s_begin, i64 s_end, int unit,
                                         RowWalk &w) {
    const unsigned wave = __builtin_amdgcn_readfirstlane(
        blockIdx.x * (SWEEP_BLOCK >> 6) + (threadIdx.x >> 6));
    return unit_enter(wave, s_begin, s_end, unit, w);
}
// the step after a row of the static schedule
__device__ __forceinline__ i64 row_next(i64 s, i64 s_begin, i64 s_end,
                                        int unit, unsigned waves, RowWalk &w) {
    if (++w.row < w.row_end) return s + 64;
    return unit_enter(waves + w.k, s_begin, s_end, unit, w);
}
// The queue's ticket is taken in two halves, so that its round trip is not
// paid on its own at the unit's end. queue_request runs in the last row of a
// unit, right after that row's first loads have been issued: lane 0 asks for
// the next queued unit of this block's head h, and the wait for the answer
// is the wait for those loads. row_next, after the row, turns the answer
// into a unit: the i-th ticket of head h is queued unit i * heads + h. A
// wave still takes exactly one ticket per unit it finishes. The answer is
// wave-uniform and costs no VGPR.
__device__ __forceinline__ unsigned queue_request(const RowQueue &q,
                                                  const RowWalk &w) {
    if (!q.ticket || w.row + 1 != w.row_end) return 0;
    unsigned long long t = 0;
    if ((threadIdx.x & 63) == 0)
        t = atomicAdd(
            q.ticket + (blockIdx.x & (q.heads - 1)) * QUEUE_HEAD_STRIDE,
            1ull);
    return __builtin_amdgcn_readfirstlane((unsigned)t);
}
__device__ __forceinline__ i64 row_next(i64 s, i64 s_begin, i64 s_end,
                                        const RowQueue &q, unsigned waves,
                                        unsigned ticket, RowWalk &w) {
    if (++w.row < w.row_end) return s + 64;
    unsigned k = w.k;
    if (q.ticket) {
        const unsigned h = blockIdx.x & (q.heads - 1);
        k = (ticket - q.base[h]) * q.heads + h;
    }
    return unit_enter(waves + k, s_begin, s_end, q.unit, w);
}

// A load that stays where it is written. The compiler sinks a plain load
// into the branch that holds its only uses; for chunk_off that is the
// deg != 0 side, one round trip later than the address was known. A relaxed
// wavefront-scope atomic load is an ordinary global_load that is not moved.
__device__ __forceinline__ i64 load_in_place(const i64 *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// ---- K4 general sweep: LDS slots + spill, any iteration ----
// IDP: perm is the identity (mv_graph_state::perm_identity), so a position
// is its vertex and the row starts without the perm round trip.
// The row's loads are ordered by when their values are needed, not by where
// they are used: chunk_off (a function of the position alone) goes out with
// perm; deg, vcurr and, for weighted graphs, vDegree in the next trip (a
// unit graph's vDegree is (double)deg, K1), and with them the queue's
// ticket; cinfo[cc], which only the gain scan reads, with the first tail
// loads, so that it travels under the edge loop. The tails stay guarded by
// deg: the SELL padding is never written and
// a trailing slice of isolated vertices has width 0.
//
// Slots. A weighted lane keeps slot t as a f64 sum at sacc[t * B + tid] and a
// u32 key at skey[t * B + tid]: 12 B, two LDS trips on a hit. On a unit graph
// every accumulated weight is 1.0, so a slot sum is an integer count, exact
// in any order, and (double)count carries the bits the f64 sum would: the
// UNIT slot is one uint2 {key, count} at spair[t * B + tid] — 8 B, one
// ds_read_b64 per probe, an integer add on a hit. The spill region keeps its
// u32 keys and f64 sums in both forms.
// UNIT also takes the self-loop test and the own-community sum out of the
// ordered edge loop: each accumulator sees its own additions in the same
// order wherever they are issued, so an unrolled pass over the chunk counts
// both (as integers) and the rolled loop reads nothing but cb[j]. The
// weighted body accumulates in edge order inside the loop, as the reference
// does. The UNIT probe has no per-lane break: it reads the lane's ns slots
// and keeps the match, and one masked store writes the hit's new count. A
// wave walks its longest lane's slots either way; without the break the
// exec-mask bookkeeping of the loop's two exits is gone (measured:
// experiments/RESULTS.md, "Unit counts").
constexpr int sweep_slot_bytes(bool unit) { return unit ? 8 : 12; }
// dynamic LDS of a k4_sweep block: the launch and the occupancy query
constexpr size_t sweep_lds_bytes(int slots, bool unit) {
    return (size_t)slots * SWEEP_BLOCK * sweep_slot_bytes(unit);
}

template <bool MR, int SLOTS, bool UNIT, bool IDP>
__global__ __launch_bounds__(SWEEP_BLOCK)
__attribute__((amdgpu_waves_per_eu(UNIT ? 6 : 5)))
void k4_sweep(
    i64 s_begin, i64 s_end, i64 lnv, i64 base,
    const unsigned *__restrict__ perm,
    const unsigned *__restrict__ deg_int, const i64 *__restrict__ chunk_off,
    const int *__restrict__ sell_tidx, const double *__restrict__ sell_w,
    const unsigned *__restrict__ vcurr, const unsigned *__restrict__ vghost,
    const double *__restrict__ vDegree, const unsigned *__restrict__ sigma,
    const Cinfo *__restrict__ cinfo, Cinfo *__restrict__ cupd,
    const i64 *__restrict__ rc_ids,
    const Info16 *__restrict__ rc_info, Info16 *__restrict__ rcu,
    double constant, unsigned *__restrict__ vtarget,
    double *__restrict__ clusterWeight, unsigned *__restrict__ spill_keys,
    double *__restrict__ spill_acc, const i64 *__restrict__ spill_off,
    RowQueue queue) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int B = SWEEP_BLOCK;
    // one of the two slot forms is live in an instantiation
    double *sacc = reinterpret_cast<double *>(smem);
    unsigned *skey =
        reinterpret_cast<unsigned *>(smem + sizeof(double) * SLOTS * B);
    uint2 *spair = reinterpret_cast<uint2 *>(smem);
    const int tid = threadIdx.x;
    const i64 gthread = blockIdx.x * (i64)B + threadIdx.x;
    unsigned *myspill_k = spill_keys + spill_off[gthread];
    double *myspill_a = spill_acc + spill_off[gthread];
    const unsigned waves = sweep_waves();

    RowWalk walk;
    for (i64 s = row_first(s_begin, s_end, queue.unit, walk); s < s_end;) {
        const i64 coff = load_in_place(chunk_off + (s >> 6));
        const i64 i = IDP ? (unsigned)s : perm[s]; // internal vertex index
                                                   // (lnv < 2^32)
        const int deg = (int)deg_int[i];
        const unsigned cc = vcurr[i];
        double vdeg = 0.0;
        if (!UNIT) vdeg = vDegree[i];
        const unsigned ticket = queue_request(queue, walk);
        const i64 ebase = coff + (s & 63);
        unsigned target;
        if (deg == 0) {
            target = cc;          // dspl.hpp:323-324
            clusterWeight[i] = 0; // K5 semantics (dspl.hpp:481-482)
        } else {
            if (UNIT) vdeg = (double)deg;
            double c0 = 0.0, selfLoop = 0.0;
            unsigned c0_n = 0, self_n = 0; // UNIT: the two sums as counts
            int ns = 0, nspill = 0;
            int tb[CH];
            double wb[CH];
            int m = min(CH, deg);
            load_tails<UNIT>(ebase, 0, m, sell_tidx, sell_w, tb, wb);
            const Cinfo cci = comm_info<MR>(cc, lnv, cinfo, rc_info);
            for (int k0 = 0;;) {
                unsigned cb[CH];
                gather_comms<MR>(tb, lnv, vcurr, vghost, cb);
                if constexpr (UNIT) {
#pragma unroll
                    for (int j = 0; j < CH; j++) {
                        self_n += j < m && (i64)tb[j] == i; // dspl.hpp:247-248
                        c0_n += j < m && cb[j] == cc;
                    }
                }
                for (int j = 0; j < m; j++) {
                    const double w = UNIT ? 1.0 : wb[j];
                    const unsigned tcomm = cb[j];
                    if constexpr (UNIT) {
                        if (tcomm == cc) continue;
                    } else {
                        if ((i64)tb[j] == i) selfLoop += w; // :247-248
                        if (tcomm == cc) { c0 += w; continue; }
                    }
                    bool found = false;
                    if constexpr (UNIT) {
                        // no break: scan the lane's ns slots, keep the match
                        int hit = -1;
                        unsigned hit_n = 0;
                        for (int t = 0; t < ns; t++) {
                            const uint2 p = spair[t * B + tid];
                            if (p.x == tcomm) {
                                hit = t;
                                hit_n = p.y;
                            }
                        }
                        if (hit >= 0) {
                            spair[hit * B + tid].y = hit_n + 1;
                            continue;
                        }
                    } else {
                        for (int t = 0; t < ns; t++) {
                            if (skey[t * B + tid] == tcomm) {
                                sacc[t * B + tid] += w;
                                found = true;
                                break;
                            }
                        }
                        if (found) continue;
                    }
                    if (ns < SLOTS) {
                        if constexpr (UNIT) {
                            spair[ns * B + tid] = make_uint2(tcomm, 1u);
                        } else {
                            skey[ns * B + tid] = tcomm;
                            sacc[ns * B + tid] = w;
                        }
                        ns++;
                        continue;
                    }
                    for (int t = 0; t < nspill; t++) {
                        if (myspill_k[t] == tcomm) {
                            myspill_a[t] += w;
                            found = true;
                            break;
                        }
                    }
                    if (!found) { // spill_max covers the max degree
                        myspill_k[nspill] = tcomm;
                        myspill_a[nspill] = w;
                        nspill++;
                    }
                }
                k0 += CH;
                if (k0 >= deg) break;
                m = min(CH, deg - k0);
                load_tails<UNIT>(ebase, k0, m, sell_tidx, sell_w, tb, wb);
            }
            if constexpr (UNIT) { // counts of 1.0: the sums' exact bits
                c0 = (double)c0_n;
                selfLoop = (double)self_n;
            }
            clusterWeight[i] = c0; // dspl.hpp:318 onto the K5-zeroed value

            // distGetMaxIndex: LDS slots first, then the spill in
            // insertion order — two loops, so that the slots are plain LDS
            // reads (one loop selecting between the two address spaces
            // compiles to flat loads waited for as vector memory)
            const double eix = c0 - selfLoop;
            const double ax = cci.degree - vdeg;
            double maxGain = 0.0;
            unsigned maxIndex = cc;
            i64 maxSize = cci.size;
            for (int t = 0; t < ns; t++) {
                unsigned y;
                double eiy;
                if constexpr (UNIT) {
                    const uint2 p = spair[t * B + tid];
                    y = p.x;
                    eiy = (double)p.y;
                } else {
                    y = skey[t * B + tid];
                    eiy = sacc[t * B + tid];
                }
                argmax_step<MR>(y, eiy, eix, vdeg, ax, constant, lnv, base,
                                sigma, cinfo, rc_ids, rc_info, maxGain,
                                maxIndex, maxSize);
            }
            for (int t = 0; t < nspill; t++)
                argmax_step<MR>(myspill_k[t], myspill_a[t], eix, vdeg, ax,
                                constant, lnv, base, sigma, cinfo, rc_ids,
                                rc_info, maxGain, maxIndex, maxSize);
            target = singleton_guard<MR>(maxIndex, maxSize, cc, cci.size, lnv,
                                         base, sigma, rc_ids);
        }

        if (target != cc) // deg > 0 here, so vdeg is the vertex's
            move_update<MR, MR>(cc, target, vdeg, lnv, cupd, rcu);
        vtarget[i] = target; // dspl.hpp:404 (view; persisted as a label)
        s = row_next(s, s_begin, s_end, queue, waves, ticket, walk);
    }
}

// ---- K4 high-degree path (wave-per-vertex) ----
// For skewed graphs (Orkut-class hubs), one WAVE processes one vertex:
// lanes stride the CSR row (coalesced 8-B tails), aggregate into a
// per-vertex open-addressed hash in HBM (L2-resident; u32 view keys CASed
// from ~0, weights atomicAdd), then a wave-reduce argmax applies the
// reference tie-break (wave_reduce_best). Unit-weight graphs only: their sums are integer-exact under
// any accumulation order; -w skewed graphs take the serial lane path
// instead (edge-order bit parity). tidx32 holds pre-translated internal
// indices (at p==1 a global tail id IS the local vertex id).
template <bool MR>
__global__ __launch_bounds__(256) void k4_sweep_hi(
    i64 nhi, i64 lnv, i64 base, const unsigned *__restrict__ perm,
    const unsigned *__restrict__ deg_int, const unsigned *__restrict__ sigma,
    const i64 *__restrict__ xadj, const int *__restrict__ tidx32,
    const unsigned *__restrict__ vcurr, const unsigned *__restrict__ vghost,
    const double *__restrict__ vDegree, const Cinfo *__restrict__ cinfo,
    Cinfo *__restrict__ cupd, const i64 *__restrict__ rc_ids,
    const Info16 *__restrict__ rc_info, Info16 *__restrict__ rcu,
    double constant, unsigned *__restrict__ vtarget,
    double *__restrict__ clusterWeight, const i64 *__restrict__ hash_off,
    i64 *__restrict__ hkeys, double *__restrict__ hacc) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;
    for (i64 s = (i64)blockIdx.x * wpb + wid; s < nhi;
         s += (i64)gridDim.x * wpb) {
        const i64 i = perm[s];
        const i64 v = sigma[i];
        const int deg = (int)deg_int[i];
        const i64 e0 = xadj[v];
        const unsigned cc = vcurr[i];
        const i64 hoff = hash_off[s];
        const i64 cap = hash_off[s + 1] - hoff; // power of two
        const Cinfo cci = comm_info<MR>(cc, lnv, cinfo, rc_info);
        double c0 = 0.0, selfLoop = 0.0;
        for (int k = lane; k < deg; k += 64) {
            const i64 ti = tidx32[e0 + k]; // pre-translated internal index
            const double w = 1.0;          // hub path is unit-only
            if (ti == i) selfLoop += w;
            const unsigned tcomm = (!MR || ti < lnv) ? vcurr[ti]
                                                     : vghost[ti - lnv];
            if (tcomm == cc) { c0 += w; continue; }
            i64 pos = hash_start(tcomm, cap);
            for (;;) {
                const i64 prev = (i64)atomicCAS(
                    (unsigned long long *)&hkeys[hoff + pos],
                    (unsigned long long)(-1ll), (unsigned long long)tcomm);
                if (prev == -1 || prev == (i64)tcomm) {
                    atomicAdd(&hacc[hoff + pos], w);
                    break;
                }
                pos = (pos + 1) & (cap - 1);
            }
        }
        // wave sums (integer-exact for unit weights)
        for (int off = 32; off > 0; off >>= 1) {
            c0 += __shfl_down(c0, off, 64);
            selfLoop += __shfl_down(selfLoop, off, 64);
        }
        c0 = __shfl(c0, 0, 64);
        selfLoop = __shfl(selfLoop, 0, 64);
        const double vdeg = vDegree[i];
        const double eix = c0 - selfLoop;
        const double ax = cci.degree - vdeg;
        // per-lane best over the hash slots, then the wave reduce
        double bg = 0.0;
        i64 bl = INT64_MAX, bs = 0;
        for (i64 t = lane; t < cap; t += 64) {
            const i64 yk = hkeys[hoff + t];
            if (yk == -1) continue;
            const unsigned y = (unsigned)yk;
            const double eiy = hacc[hoff + t];
            const Cinfo c = comm_info<MR>(y, lnv, cinfo, rc_info);
            const double g = dq_gain(eiy, eix, vdeg, c.degree, ax, constant);
            const i64 yh =
                ((i64)label_of<MR>(y, lnv, base, sigma, rc_ids) << 32) |
                (i64)y;
            if (g > bg || (g == bg && g != 0.0 && yh < bl)) {
                bg = g;
                bl = yh;
                bs = c.size;
            }
        }
        wave_reduce_best(bg, bl, bs);
        if (lane == 0) {
            const label_t<MR> ccLabel =
                label_of<MR>(cc, lnv, base, sigma, rc_ids);
            unsigned target =
                (bl == INT64_MAX) ? cc : (unsigned)(bl & 0xffffffffu);
            const label_t<MR> tLabel =
                (bl == INT64_MAX) ? ccLabel : (label_t<MR>)(bl >> 32);
            if (bs == 1 && cci.size == 1 && tLabel > ccLabel)
                target = cc; // :224-225
            if (deg == 0) {
                clusterWeight[i] = 0;
                target = cc;
            } else {
                clusterWeight[i] = c0;
            }
            if (target != cc)
                move_update<MR, MR>(cc, target, vdeg, lnv, cupd, rcu);
            vtarget[i] = target;
        }
    }
}

// ---- K4 lane-hash path (skewed graphs, mid/high-degree band) ----
// One LANE per vertex — accumulation stays in edge order, bit-exact for
// -w (dspl.hpp:240-271) — with the clmap as an open-addressed per-VERTEX
// hash (d_hash_off regions) PLUS a compact candidate list (d_lh_list):
// O(1) expected insert/lookup instead of the LDS path's O(ncand) linear
// probe per edge, and the argmax scans exactly ncand entries (in insertion
// order) instead of the whole hash capacity. This is the aggregation
// structure for vertices whose persistent distinct-candidate count exceeds
// the LDS slots (long-range-edge-heavy social graphs). One view-form
// instantiation per UNIT serves p==1 too (the slot array IS the view).
template <bool UNIT>
__global__ __launch_bounds__(256) void k4_sweep_lh(
    i64 s_begin, i64 s_end, i64 lnv, i64 base,
    const unsigned *__restrict__ perm,
    const unsigned *__restrict__ deg_int, const i64 *__restrict__ chunk_off,
    const int *__restrict__ sell_tidx, const double *__restrict__ sell_w,
    const unsigned *__restrict__ vcurr, const unsigned *__restrict__ vghost,
    const double *__restrict__ vDegree, const unsigned *__restrict__ sigma,
    const Cinfo *__restrict__ cinfo, Cinfo *__restrict__ cupd,
    const i64 *__restrict__ rc_ids, const Info16 *__restrict__ rc_info,
    Info16 *__restrict__ rcu, double constant,
    unsigned *__restrict__ vtarget, double *__restrict__ clusterWeight,
    const i64 *__restrict__ hash_off, i64 *__restrict__ hkeys,
    double *__restrict__ hacc, unsigned *__restrict__ lh_list) {
    constexpr bool MR = true;
    const i64 gthread = blockIdx.x * (i64)blockDim.x + threadIdx.x;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 s = s_begin + gthread; s < s_end; s += stride) {
        const i64 i = perm[s];
        const int deg = (int)deg_int[i];
        const i64 ebase = chunk_off[s >> 6] + (s & 63);
        const unsigned cc = vcurr[i];
        const i64 hoff = hash_off[s];
        const i64 cap = hash_off[s + 1] - hoff; // power of two
        unsigned *mylist = lh_list + (hoff >> 1); // cap/2 >= deg entries
        const Cinfo cci = comm_info<MR>(cc, lnv, cinfo, rc_info);
        double c0 = 0.0, selfLoop = 0.0;
        int ncand = 0;
        for (int k0 = 0; k0 < deg; k0 += CH) {
            const int m = min(CH, deg - k0);
            i64 tb[CH];
            unsigned cb[CH];
            double wb[CH];
            load_chunk<MR, UNIT>(ebase, k0, m, lnv, sell_tidx, sell_w, vcurr,
                                 vghost, tb, wb, cb);
            for (int j = 0; j < m; j++) {
                const double w = UNIT ? 1.0 : wb[j];
                if (tb[j] == i) selfLoop += w; // dspl.hpp:247-248
                const unsigned tcomm = cb[j];
                if (tcomm == cc) { c0 += w; continue; }
                i64 pos = hash_start(tcomm, cap);
                for (;;) {
                    const i64 key = hkeys[hoff + pos];
                    if (key == (i64)tcomm) {
                        hacc[hoff + pos] += w; // edge-order: one lane owns
                        break;                 // this vertex
                    }
                    if (key == -1) {
                        hkeys[hoff + pos] = tcomm;
                        hacc[hoff + pos] = w;
                        mylist[ncand++] = (unsigned)pos;
                        break;
                    }
                    pos = (pos + 1) & (cap - 1);
                }
            }
        }
        clusterWeight[i] = c0; // dspl.hpp:318

        // distGetMaxIndex over the compact list
        const double vdeg = vDegree[i];
        const double eix = c0 - selfLoop;
        const double ax = cci.degree - vdeg;
        double maxGain = 0.0;
        unsigned maxIndex = cc;
        i64 maxSize = cci.size;
        for (int t = 0; t < ncand; t++) {
            const i64 pos = mylist[t];
            argmax_step<MR>((unsigned)hkeys[hoff + pos], hacc[hoff + pos],
                            eix, vdeg, ax, constant, lnv, base, sigma, cinfo,
                            rc_ids, rc_info, maxGain, maxIndex, maxSize);
        }
        unsigned target = singleton_guard<MR>(maxIndex, maxSize, cc, cci.size,
                                              lnv, base, sigma, rc_ids);
        if (deg == 0) target = cc;
        if (target != cc)
            move_update<MR, MR>(cc, target, vdeg, lnv, cupd, rcu);
        vtarget[i] = target;
    }
}

// ---- K4 first-iteration specialization ----
// At iteration 1 currComm is the identity (dspl.hpp:145-147), so per vertex:
// counter[0] collects exactly the self-loop weight (eix = counter[0] -
// selfLoop == 0.0, dspl.hpp:183), ax = ccDegree - vDegree == 0.0 (:185),
// every community has size 1, and each distinct neighbor TAIL is its own
// candidate — no community gather at all. With per-row tails sorted
// ascending (the reference CSR's order, graph.hpp:1145-1153 — verified at
// load), parallel edges are adjacent and candidates arrive in ascending
// label order, so the tie-break (max gain, then smallest label,
// dspl.hpp:214-215) reduces to a strict-greater streaming argmax: no clmap
// at all. A LOCAL candidate's view is its tail index and its degree ay is
// vDegree[tidx] — a spatially local gather instead of a random cinfo line;
// a ghost candidate's view comes from vghost (already lnv + rc index — the
// old per-edge rc binary search disappears). The singleton guard
// (dspl.hpp:224-225) is the final maxLabel > ccLabel check, on labels that
// come batched from sigma / the sorted ghost id list. Gains carry the
// identical bits: dq_gain with eix = ax = 0.0 rounds exactly like the
// reference's expressions (x - 0.0 == x).
// LBL_ASC: rows are label-ascending (the reference CSR order), so the
// strict-greater argmax implicitly keeps the smallest label on gain ties.
// With internal-sorted rows (k_sell_sort_rows) candidates stream in
// INTERNAL order instead and ties compare the batched labels explicitly.
// IDP and the order of the row's first loads: as in k4_sweep.
template <bool MR, bool UNIT, bool LBL_ASC, bool IDP>
__global__ __launch_bounds__(SWEEP_BLOCK) void k4_sweep_iter1(
    i64 s_begin, i64 s_end, i64 lnv, i64 base,
    const unsigned *__restrict__ perm,
    const unsigned *__restrict__ deg_int, const i64 *__restrict__ chunk_off,
    const int *__restrict__ sell_tidx, const double *__restrict__ sell_w,
    const unsigned *__restrict__ vghost, const i64 *__restrict__ ghosts,
    const double *__restrict__ vDegree, const unsigned *__restrict__ sigma,
    Cinfo *__restrict__ cupd,
    const Info16 *__restrict__ rc_info, Info16 *__restrict__ rcu,
    double constant, unsigned *__restrict__ vtarget,
    double *__restrict__ clusterWeight, int S_rows) {
    using label = label_t<MR>;
    const unsigned waves = sweep_waves();
    RowWalk walk;
    for (i64 s = row_first(s_begin, s_end, S_rows, walk); s < s_end;
         s = row_next(s, s_begin, s_end, S_rows, waves, walk)) {
        const i64 coff = load_in_place(chunk_off + (s >> 6));
        const i64 i = IDP ? (unsigned)s : perm[s]; // lnv < 2^32
        const int deg = (int)deg_int[i];
        const i64 ebase = coff + (s & 63);
        const unsigned cc = (unsigned)i; // own slot (identity)
        const label ccLabel = own_label<MR>(i, base, sigma);
        // a unit graph's vDegree is the row length (K1)
        const double vdeg = UNIT ? (double)deg : vDegree[i];
        double c0 = 0.0;
        double maxGain = 0.0;
        unsigned maxIndex = cc;
        label maxLabel = ccLabel;
        i64 prev = INT64_MIN;
        unsigned pend_view = 0;
        label pend_label = 0;
        double eiy = 0.0, pend_ay = 0.0;
        bool pend = false;
        auto close_pending = [&] { // the pending candidate is complete
            const double g = dq_gain(eiy, 0.0, vdeg, pend_ay, 0.0, constant);
            if (g > maxGain) {
                maxGain = g;
                maxIndex = pend_view;
                maxLabel = pend_label;
            } else if (!LBL_ASC && g == maxGain && g != 0.0 &&
                       pend_label < maxLabel) {
                maxIndex = pend_view; // dspl.hpp:214-215 tie
                maxLabel = pend_label;
            }
        };
        for (int k0 = 0; k0 < deg; k0 += CH) {
            const int m = min(CH, deg - k0);
            i64 tb[CH];
            label lb[CH];
            double wb[CH], vb[CH];
            load_tails<UNIT>(ebase, k0, m, sell_tidx, sell_w, tb, wb);
#pragma unroll
            for (int j = 0; j < CH; j++) {
                const bool local = !MR || tb[j] < lnv;
                lb[j] = local ? own_label<MR>(tb[j], base, sigma)
                              : (label)ghosts[clamp0(tb[j] - lnv)];
                vb[j] = local ? vDegree[tb[j]] : 0.0;
            }
            for (int j = 0; j < m; j++) {
                const i64 tidx = tb[j];
                const double w = UNIT ? 1.0 : wb[j];
                if (tidx == i) { c0 += w; continue; } // self: counter[0]
                if (tidx == prev) { eiy += w; continue; } // parallel edge
                if (pend) close_pending();
                prev = tidx;
                if (!MR || tidx < lnv) {
                    pend_view = (unsigned)tidx; // candidate comm == tail
                    pend_ay = vb[j];
                } else {
                    pend_view = vghost[tidx - lnv]; // lnv + rc index
                    pend_ay = rc_info[clamp0((i64)pend_view - lnv)].degree;
                }
                pend_label = lb[j];
                eiy = w;
                pend = true;
            }
        }
        if (pend) close_pending();
        if (maxLabel > ccLabel) maxIndex = cc; // singleton guard
        clusterWeight[i] = c0;                 // dspl.hpp:318 (eix == 0)
        if (maxIndex != cc)                    // cc is local at iteration 1
            move_update<false, MR>(cc, maxIndex, vdeg, lnv, cupd, rcu);
        vtarget[i] = maxIndex;
    }
}

// index of a k4_sweep SLOTS value in mv_sweep_info::general_slots
constexpr int mv_sweep_slot_index(int slots) {
    return slots == 4 ? 0 : slots == 8 ? 1 : slots == 12 ? 2 : slots == 16 ? 3
         : slots == 24 ? 4 : slots == 32 ? 5 : 6;
}

// ---- launch dispatch: run-time routing to the template instantiations ----
int env_int(const char *name, int unset) {
    const char *s = getenv(name);
    return s ? atoi(s) : unset;
}

// by_flag turns a run-time bool into a std::bool_constant tag
template <class F> void by_flag(bool b, F f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// What the launches of one iteration share. Mode (the kernels' MR): view
// mode at p>1; at p==1 slot mode, where the u32 slot arrays ARE the view and
// the ghost/rc pointers are load_graph's never-read dummies (d_ghosts: null).
struct Sweep {
    mv_engine *e;
    const SweepPlan &plan;
    const unsigned *vcurr;
    unsigned *vtarget;
    int slots;   // k4_sweep's SLOTS in this iteration
    bool queued; // its k4_sweep launches take their rows from the queue
};
Sweep sweep_of(mv_engine *e, const SweepPlan &plan, int iter,
               const i64 *d_curr, i64 *d_target) {
    const bool p1 = e->nranks == 1;
    return {e, plan, p1 ? (const unsigned *)d_curr : e->d_vcurr.get(),
            p1 ? (unsigned *)d_target : e->d_vtarget.get(),
            iter <= plan.first_iters ? plan.slots_first : plan.slots_rest,
            plan.queue_from && iter >= plan.queue_from};
}

int range_grid(const mv_engine *e, i64 s0, i64 s1) {
    return e->nranks == 1 ? e->sweep_grid
                          : grid_for(s1 - s0, 256, e->sweep_grid);
}

// the queue's launch view; the host totals advance by the launch's tickets
RowQueue take_queue(mv_engine *e, i64 s0, i64 s1, int grid) {
    RowQueue q{e->d_ticket, {}, e->sched_unit, 1};
    int64_t add[QUEUE_HEADS];
    q.heads = queue_tickets(s1 - s0, q.unit, grid, add);
    for (int h = 0; h < q.heads; h++) {
        q.base[h] = (unsigned)e->tickets_total[h];
        e->tickets_total[h] += add[h];
    }
    return q;
}

template <bool MR, int S, bool UNIT, bool IDP>
void launch_sweep(const Sweep &w, i64 s0, i64 s1) {
    mv_engine *e = w.e;
    const auto kernel = k4_sweep<MR, S, UNIT, IDP>;
    constexpr size_t lds = sweep_lds_bytes(S, UNIT); // S slots per lane
    e->sweep.general++;
    e->sweep.general_slots[mv_sweep_slot_index(S)]++;
    e->sweep.slot_bytes = sweep_slot_bytes(UNIT);
    int grid = range_grid(e, s0, s1);
    if (w.queued) {
        // one resident round: a first unit on a block that starts late is
        // a unit no other wave can take
        int &per_cu = e->sweep_per_cu[mv_sweep_slot_index(S)][UNIT][IDP];
        if (!per_cu) { // once per engine and instantiation
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, kernel, 256, lds));
            per_cu = std::max(per_cu, 1);
        }
        grid = std::min(grid, per_cu * e->num_cus);
    }
    if (s1 == e->lnv) e->sched_grid = grid;
    // launches that do not queue: the static schedule on the full grid
    const RowQueue static_rows{nullptr, {}, e->row_group, 0};
    kernel<<<grid, 256, lds, e->stream>>>(
        s0, s1, e->lnv, e->base, e->d_perm, e->d_deg, e->d_chunk_off,
        e->d_sell_tidx, e->d_sell_w, w.vcurr, e->d_vghost, e->d_vdeg,
        e->d_sigma, e->d_cinfo, e->d_cupd, e->d_rc_ids, e->d_rc_info,
        e->d_rcu, w.plan.constant, w.vtarget, e->d_cw,
        (unsigned *)e->d_spill_k.get(), e->d_spill_a, e->d_spill_off,
        w.queued ? take_queue(e, s0, s1, grid) : static_rows);
}

template <bool MR, int S, bool UNIT>
void launch_slots(const Sweep &w, i64 s0, i64 s1) {
    if (w.e->perm_identity) launch_sweep<MR, S, UNIT, true>(w, s0, s1);
    else launch_sweep<MR, S, UNIT, false>(w, s0, s1);
}
template <bool MR, bool UNIT>
void dispatch_slots(const Sweep &w, i64 s0, i64 s1) {
    switch (w.slots) {
    case 4: launch_slots<MR, 4, UNIT>(w, s0, s1); break;
    case 12: launch_slots<MR, 12, UNIT>(w, s0, s1); break;
    case 16: launch_slots<MR, 16, UNIT>(w, s0, s1); break;
    case 24: launch_slots<MR, 24, UNIT>(w, s0, s1); break;
    case 32: launch_slots<MR, 32, UNIT>(w, s0, s1); break;
    case 48: launch_slots<MR, 48, UNIT>(w, s0, s1); break;
    default: launch_slots<MR, 8, UNIT>(w, s0, s1); break;
    }
}

// k4_sweep_iter1 never queues: the static row-group schedule
template <bool MR, bool UNIT, bool LBL_ASC>
void launch_iter1(const Sweep &w, i64 s0, i64 s1) {
    mv_engine *e = w.e;
    if (LBL_ASC) e->sweep.iter1_label_order++;
    else e->sweep.iter1_internal_order++;
    by_flag(e->perm_identity, [&](auto idp_tag) {
        k4_sweep_iter1<MR, UNIT, LBL_ASC, decltype(idp_tag)::value>
            <<<range_grid(e, s0, s1), 256, 0, e->stream>>>(
                s0, s1, e->lnv, e->base, e->d_perm, e->d_deg, e->d_chunk_off,
                e->d_sell_tidx, e->d_sell_w, e->d_vghost, e->d_ghosts,
                e->d_vdeg, e->d_sigma, e->d_cupd, e->d_rc_info, e->d_rcu,
                w.plan.constant, w.vtarget, e->d_cw, e->row_group);
    });
}

} // namespace

// LDS slots per lane: early iterations see ~degree distinct candidate
// communities (every vertex its own community), later ones only a handful —
// a larger-slot / lower-occupancy variant for the first iterations avoids
// the spill path where it matters. Degree-adaptive defaults: RGG-class
// graphs (deg ~10) measured best at 8 slots (12 first iterations at p==1);
// dense social shapes (deg ~70, ~25 persistent distinct candidates from
// long-range edges) at 24 (72 KiB/block, 2 blocks/CU) — +23% on the
// orkut_like workload, while 32+ falls off the occupancy cliff.
// Row schedule: the queue serves k4_sweep from iteration first_iters + 1 on
// (MV_SWEEP_QUEUE_FROM moves that): while nearly every vertex moves, the
// tickets wait behind the moves' own cupd atomics and the queue loses (both
// measured, experiments/RESULTS.md).
SweepPlan sweep_plan(const mv_engine *e, double constant) {
    // the tunables, read once per process (perf only, results identical)
    static const int slots_env = env_int("MV_SLOTS", 0),
                     slots_first_env = env_int("MV_SLOTS_FIRST", -1),
                     first_iters = env_int("MV_FIRST_ITERS", 2);
    static const bool no_iter1 = getenv("MV_NO_ITER1") != nullptr;
    const bool dense = e->lne > 16 * e->lnv;
    SweepPlan plan{constant};
    plan.slots_rest = slots_env > 0 ? slots_env : (dense ? 24 : 8);
    plan.slots_first = slots_first_env > 0 ? slots_first_env
                       : dense             ? 24
                       : e->nranks == 1    ? 12
                                           : plan.slots_rest;
    plan.first_iters = first_iters;
    if (e->sched_unit > 0)
        plan.queue_from =
            std::max(e->sched_from ? e->sched_from : first_iters + 1, 1);
    if ((e->rows_sorted || e->sell_sorted) && !no_iter1)
        plan.iter1 = e->sell_sorted    ? ITER1_INTERNAL
                     : e->unit_weights ? ITER1_UNIT
                                       : ITER1_WEIGHTED;
    return plan;
}

void sweep_hash_bands(mv_engine *e, const SweepPlan &plan, int iter,
                      const i64 *d_curr, i64 *d_target) {
    if (e->nlh <= 0) return;
    const Sweep w = sweep_of(e, plan, iter, d_curr, d_target);
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv;
    HIP_CHECK(hipMemsetAsync(e->d_hkeys, 0xFF, 8 * e->hash_total, st));
    if (e->hash_hub_elems) // the wave kernel atomic-adds into its prefix;
                           // the lane band writes on insert
        HIP_CHECK(hipMemsetAsync(e->d_hacc, 0, 8 * e->hash_hub_elems, st));
    if (e->nlh > e->nhi) // per-lane hash band [nhi, nlh)
        by_flag(e->unit_weights, [&](auto unit_tag) {
            e->sweep.lh++;
            k4_sweep_lh<decltype(unit_tag)::value>
                <<<grid_for(e->nlh - e->nhi), 256, 0, st>>>(
                    e->nhi, e->nlh, lnv, e->base, e->d_perm, e->d_deg,
                    e->d_chunk_off, e->d_sell_tidx, e->d_sell_w, w.vcurr,
                    e->d_vghost, e->d_vdeg, e->d_sigma, e->d_cinfo,
                    e->d_cupd, e->d_rc_ids, e->d_rc_info, e->d_rcu,
                    plan.constant, w.vtarget, e->d_cw, e->d_hash_off,
                    e->d_hkeys, e->d_hacc, e->d_lh_list);
        });
    if (e->nhi > 0) // wave-per-vertex hubs [0, nhi)
        by_flag(e->nranks > 1, [&](auto mr_tag) {
            e->sweep.hi++;
            k4_sweep_hi<decltype(mr_tag)::value>
                <<<grid_for(e->nhi * 64, 256, 2048), 256, 0, st>>>(
                    e->nhi, lnv, e->base, e->d_perm, e->d_deg, e->d_sigma,
                    e->d_xadj, e->d_tidx32, w.vcurr, e->d_vghost, e->d_vdeg,
                    e->d_cinfo, e->d_cupd, e->d_rc_ids, e->d_rc_info,
                    e->d_rcu, plan.constant, w.vtarget, e->d_cw,
                    e->d_hash_off, e->d_hkeys, e->d_hacc);
        });
}

void sweep_positions(mv_engine *e, const SweepPlan &plan, int iter,
                     const i64 *d_curr, i64 *d_target, i64 s0, i64 s1) {
    if (s1 <= s0) return;
    const Sweep w = sweep_of(e, plan, iter, d_curr, d_target);
    by_flag(e->nranks > 1, [&](auto mr_tag) {
        constexpr bool MR = decltype(mr_tag)::value;
        switch (iter == 1 ? plan.iter1 : ITER1_GENERAL) { // <MR,UNIT,LBL_ASC>
        case ITER1_INTERNAL: launch_iter1<MR, true, false>(w, s0, s1); break;
        case ITER1_UNIT: launch_iter1<MR, true, true>(w, s0, s1); break;
        case ITER1_WEIGHTED: launch_iter1<MR, false, true>(w, s0, s1); break;
        case ITER1_GENERAL:
            if (e->unit_weights) dispatch_slots<MR, true>(w, s0, s1);
            else dispatch_slots<MR, false>(w, s0, s1);
        }
    });
}
