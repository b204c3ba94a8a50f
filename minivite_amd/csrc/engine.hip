// engine.hip — the MI355X-native Louvain phase-1 engine: CDNA4 HIP kernels
// + RCCL-over-xGMI halo exchange behind the C-ABI in include/minivite_hip.h.
//
// Drop-in for distLouvainMethod (dspl.hpp:1280-1441). Kernel inventory maps
// the reference's OpenMP regions: K1 vertex-degree sum
// (dspl.hpp:82-107), K2 constant (109-130), K3 comm iota (132-149), K4 THE
// sweep (276-405 with 230-274, 174-228), K5 zero (473-486), K6 cinfo apply
// (458-471), K7 modularity (407-456), K8 ghost-comm gather (559-571), K9
// cinfo reply gather (776-929), K10 ghost discovery (1112-1272). MPI call
// sites become grouped ncclSend/ncclRecv alltoallv over
// xGMI + ncclAllReduce for the 1-2 double reductions.
//
// Device data layout:
//  * Per-vertex working arrays (currComm/pastComm/targetComm, vDegree,
//    clusterWeight) live in INTERNAL order: a spatial permutation sigma
//    (the builder's locality hint) so that a vertex's neighbors — whose
//    GLOBAL ids the RGG assigns randomly — sit nearby in memory and the
//    per-edge community gathers hit L1/L2 instead of round-tripping to the
//    Infinity Cache (measured: the label-order layout fetched 3.5x its
//    algorithmic bytes at 13% L2 hit rate, 86% wave-wait). Community
//    LABELS, the wire protocol and every result are untouched: sigma is
//    pure layout. Without a hint, internal order = degree-sorted (load
//    balance for skewed graphs).
//  * Edges: SELL-64 (sliced ELL, slice = one wave64) over internal order;
//    edge step k of a wave loads 64 consecutive int32 pre-translated tails
//    (local -> internal index, ghost -> lnv + slot in the sorted ghost
//    list) — one coalesced 256-B line pair per wave-instruction, replacing
//    the reference's 16-B AoS row walk (graph.hpp:60-66) and per-edge hash
//    lookup (dspl.hpp:253-260). Unit-weight graphs skip the weight stream
//    entirely (every w == 1.0, detected at load).
//  * Community info (localCinfo/localCupdate, dspl.hpp:61-66) is AoS
//    {int64 size; double degree} in INTERNAL order. Persistent community
//    arrays carry LABELS; sweeps run over u32 slot (p==1) / view (p>1)
//    encodings that index cinfo/rc_info directly (see k_build_view).
//
// FP discipline: built with -ffp-contract=off so the dQ gain expression
// (dspl.hpp:212) and all accumulations carry the same bits as the
// gcc-built reference / oracle (generic x86-64 has no FMA contraction).
// Per-vertex weight accumulation is sequential in edge order (one lane owns
// one vertex), matching dspl.hpp:240-271 exactly.
//
// This is GPU-only code: engine creation fails loudly without a device.
// There is no CPU fallback anywhere in this file.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

#include "../../include/minivite_hip.h"
#include "coarsen.h"

#define HIP_CHECK(x)                                                          \
    do {                                                                      \
        hipError_t _e = (x);                                                  \
        if (_e != hipSuccess) {                                               \
            std::fprintf(stderr, "HIP error %s at %s:%d: %s\n",               \
                         hipGetErrorString(_e), __FILE__, __LINE__, #x);      \
            std::abort();                                                     \
        }                                                                     \
    } while (0)

#define NCCL_CHECK(x)                                                         \
    do {                                                                      \
        ncclResult_t _e = (x);                                                \
        if (_e != ncclSuccess) {                                              \
            std::fprintf(stderr, "RCCL error %s at %s:%d: %s\n",              \
                         ncclGetErrorString(_e), __FILE__, __LINE__, #x);     \
            std::abort();                                                     \
        }                                                                     \
    } while (0)

namespace {

using i64 = int64_t;

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

__device__ __forceinline__ i64 dev_lower_bound(const i64 *a, i64 n, i64 key) {
    i64 lo = 0, hi = n;
    while (lo < hi) {
        i64 mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ i64 dev_bsearch(const i64 *a, i64 n, i64 key) {
    i64 p = dev_lower_bound(a, n, key);
    return (p < n && a[p] == key) ? p : -1;
}

__device__ __forceinline__ void atomic_add_i64(i64 *p, i64 v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p),
              static_cast<unsigned long long>(v));
}

// ---- K1: vDegree + localCinfo init (dspl.hpp:82-107); both
// internal-ordered ----
__global__ void k1_vertex_degree(i64 lnv, const unsigned *__restrict__ sigma,
                                 const i64 *__restrict__ xadj,
                                 const double *__restrict__ ew, int unit,
                                 double *__restrict__ vDegree,
                                 Cinfo *__restrict__ cinfo) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < lnv;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 v = sigma[k];
        const i64 e0 = xadj[v], e1 = xadj[v + 1];
        double tw;
        if (unit) {
            tw = (double)(e1 - e0); // unit weights: exact
        } else {
            tw = 0.0;
            for (i64 e = e0; e < e1; e++) tw += ew[e]; // sequential edge order
        }
        vDegree[k] = tw;
        cinfo[k] = {1, tw}; // dspl.hpp:104-105 (internal slot k)
    }
}

// block-partial sum for K2/K7 (deterministic: fixed block ranges, fixed
// shuffle tree; partials summed on host in block order)
template <typename F>
__global__ void k_partial_sum2(i64 n, F f, double *__restrict__ out2) {
    double a = 0.0, b = 0.0;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x) {
        double x, y;
        f(i, x, y);
        a += x;
        b += y;
    }
    __shared__ double sa[256], sb[256];
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sa[threadIdx.x] += sa[threadIdx.x + s];
            sb[threadIdx.x] += sb[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out2[2 * blockIdx.x] = sa[0];
        out2[2 * blockIdx.x + 1] = sb[0];
    }
}

// ---- K3: community iota (dspl.hpp:132-149): internal slot k holds the
// LABEL of the vertex it represents (multi-rank arrays carry labels) ----
__global__ void k3_init_comm(i64 lnv, i64 base,
                             const unsigned *__restrict__ sigma,
                             i64 *__restrict__ curr, i64 *__restrict__ past) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < lnv;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 l = (i64)sigma[k] + base;
        curr[k] = l;
        past[k] = l;
    }
}

// ---- K10a: tag remote tails (exchangeVertexReqs, dspl.hpp:1140-1164) ----
__global__ void k_select_remote(i64 lne, const i64 *__restrict__ tails,
                                i64 base, i64 bound, i64 *__restrict__ out,
                                unsigned long long *__restrict__ count) {
    for (i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x; e < lne;
         e += (i64)gridDim.x * blockDim.x) {
        const i64 t = tails[e];
        if (t < base || t >= bound) out[atomicAdd(count, 1ull)] = t;
    }
}

// ---- SELL build (per run, setup span) ----
__global__ void k_degrees(i64 lnv, const unsigned *__restrict__ sigma,
                          const i64 *__restrict__ xadj,
                          unsigned *__restrict__ deg) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < lnv;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 v = sigma[k];
        deg[k] = (unsigned)(xadj[v + 1] - xadj[v]);
    }
}

__global__ void k_iota32(i64 n, unsigned *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x)
        out[i] = (unsigned)i;
}

__global__ void k_invert_perm(i64 n, const unsigned *__restrict__ perm,
                              unsigned *__restrict__ inv) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < n;
         i += (i64)gridDim.x * blockDim.x)
        inv[perm[i]] = (unsigned)i;
}

// slice widths: chunk c spans 64 SELL positions, width = its max degree;
// emitted as element counts (width*64)
__global__ void k_chunk_sizes(i64 nchunks, i64 lnv,
                              const unsigned *__restrict__ perm,
                              const unsigned *__restrict__ deg,
                              i64 *__restrict__ sizes) {
    for (i64 c = blockIdx.x * (i64)blockDim.x + threadIdx.x; c < nchunks;
         c += (i64)gridDim.x * blockDim.x) {
        unsigned w = 0;
        const i64 s1 = min(c * 64 + 64, lnv);
        for (i64 s = c * 64; s < s1; s++) w = max(w, deg[perm[s]]);
        sizes[c] = (i64)w * 64;
    }
}

// translate + scatter this rank's CSR rows into the SELL image
__global__ void k_fill_sell(i64 lnv, const unsigned *__restrict__ perm,
                            const unsigned *__restrict__ sigma,
                            const unsigned *__restrict__ sigma_inv,
                            const i64 *__restrict__ xadj,
                            const i64 *__restrict__ tails,
                            const double *__restrict__ w, i64 base, i64 bound,
                            const i64 *__restrict__ ghosts, i64 nghost,
                            const i64 *__restrict__ chunk_off,
                            int *__restrict__ sell_tidx,
                            double *__restrict__ sell_w) {
    for (i64 s = blockIdx.x * (i64)blockDim.x + threadIdx.x; s < lnv;
         s += (i64)gridDim.x * blockDim.x) {
        const i64 iint = perm[s];
        const i64 v = sigma[iint];
        const i64 off = chunk_off[s >> 6];
        const int l = (int)(s & 63);
        const i64 e0 = xadj[v], e1 = xadj[v + 1];
        for (i64 e = e0; e < e1; e++) {
            const i64 t = tails[e];
            const i64 ti = (t >= base && t < bound)
                               ? (i64)sigma_inv[t - base]
                               : lnv + dev_lower_bound(ghosts, nghost, t);
            const i64 slot = off + (e - e0) * 64 + l;
            sell_tidx[slot] = (int)ti;
            if (sell_w) sell_w[slot] = w[e];
        }
    }
}

__global__ void k_scatter_mark(i64 n, const unsigned *__restrict__ idx,
                               unsigned char *__restrict__ mark) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x)
        mark[idx[k]] = 1;
}

__global__ void k_gather_flags(i64 lnv, const unsigned *__restrict__ perm,
                               const unsigned char *__restrict__ mark,
                               unsigned char *__restrict__ flags,
                               int invert) {
    for (i64 s = blockIdx.x * (i64)blockDim.x + threadIdx.x; s < lnv;
         s += (i64)gridDim.x * blockDim.x)
        flags[s] = mark[perm[s]] ^ invert;
}

__global__ void k_spill_uniform(i64 nthreads, i64 per,
                                i64 *__restrict__ off) {
    for (i64 t = blockIdx.x * (i64)blockDim.x + threadIdx.x; t < nthreads;
         t += (i64)gridDim.x * blockDim.x)
        off[t] = t * per;
}

// Per-row insertion sort of the SELL image by INTERNAL tail index.
// UNIT graphs only: their per-community sums are integer-exact under any
// accumulation order and the argmax tie-break is a total order on labels,
// so edge order cannot change any result — while ascending gather
// addresses inside the sigma spatial window raise L1/L2 line reuse
// (measured +4.7% on the steady-state harness, experiments/RESULTS.md).
// -w graphs keep the reference's edge order (bit-exact accumulation).
__global__ void k_sell_sort_rows(i64 lnv, const unsigned *__restrict__ perm,
                                 const unsigned *__restrict__ deg_int,
                                 const i64 *__restrict__ chunk_off,
                                 int *__restrict__ sell_tidx) {
    for (i64 s = blockIdx.x * (i64)blockDim.x + threadIdx.x; s < lnv;
         s += (i64)gridDim.x * blockDim.x) {
        const int d = (int)deg_int[perm[s]];
        const i64 eb = chunk_off[s >> 6] + (s & 63);
        for (int k = 1; k < d; k++) {
            const int v = sell_tidx[eb + (i64)k * 64];
            int j = k - 1;
            while (j >= 0) {
                const int u = sell_tidx[eb + (i64)j * 64];
                if (u <= v) break;
                sell_tidx[eb + (i64)(j + 1) * 64] = u;
                j--;
            }
            sell_tidx[eb + (i64)(j + 1) * 64] = v;
        }
    }
}

// per-thread spill extents for skewed graphs: with the degree-DESCENDING
// SELL order, grid-stride thread t's largest vertex is its first position,
// so its spill need is max(deg_sorted[t] - min_slots, 1); offsets are the
// host-side prefix sum of these
__global__ void k_spill_need(i64 nthreads, i64 s_begin, i64 lnv,
                             const unsigned *__restrict__ perm,
                             const unsigned *__restrict__ deg, int min_slots,
                             i64 *__restrict__ need) {
    for (i64 t = blockIdx.x * (i64)blockDim.x + threadIdx.x; t < nthreads;
         t += (i64)gridDim.x * blockDim.x) {
        i64 n = 1;
        if (s_begin + t < lnv) {
            const i64 d = (i64)deg[perm[s_begin + t]] - min_slots;
            n = d > 1 ? d : 1;
        }
        need[t] = n;
    }
}

// translate the full CSR tail array into int32 internal indices (local ->
// internal slot, ghost -> lnv + ghost index) once at build: the hub wave
// kernels walk CSR rows and would otherwise pay sigma_inv[tails[e]] — two
// dependent random gathers — per edge per iteration
__global__ void k_translate_tails(i64 lne, const i64 *__restrict__ tails,
                                  i64 base, i64 bound,
                                  const unsigned *__restrict__ sigma_inv,
                                  const i64 *__restrict__ ghosts, i64 nghost,
                                  i64 lnv, int *__restrict__ out) {
    for (i64 e = blockIdx.x * (i64)blockDim.x + threadIdx.x; e < lne;
         e += (i64)gridDim.x * blockDim.x) {
        const i64 t = tails[e];
        out[e] = (t >= base && t < bound)
                     ? (int)sigma_inv[t - base]
                     : (int)(lnv + dev_lower_bound(ghosts, nghost, t));
    }
}

// translate a global-id list into internal indices (svdata, once per run)
__global__ void k_to_internal(i64 n, const i64 *__restrict__ gids, i64 base,
                              const unsigned *__restrict__ sigma_inv,
                              unsigned *__restrict__ out) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x)
        out[k] = sigma_inv[gids[k] - base];
}

// ---- the u32 community VIEW (multi-rank sweeps) ----
// Persistent community arrays carry LABELS (the reference's community ids,
// global vertex ids). Each iteration builds a u32 view: a local community
// is its home vertex's internal SLOT (< lnv, indexes cinfo/cupd directly),
// a remote one is lnv + its index in the sorted rc_ids array (indexes
// rc_info/rcu directly). The per-edge community gather halves to 4 B and
// the gain scan's per-candidate binary search disappears; only the
// tie-break needs label ORDER, fetched lazily (see the K4 note).
__global__ void k_build_view(i64 n, const i64 *__restrict__ labels, i64 base,
                             i64 bound, i64 lnv,
                             const unsigned *__restrict__ sigma_inv,
                             const i64 *__restrict__ rc_ids, i64 nrc,
                             unsigned *__restrict__ view) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 l = labels[k];
        view[k] = (l >= base && l < bound)
                      ? sigma_inv[l - base]
                      : (unsigned)(lnv + clamp0(dev_bsearch(rc_ids, nrc, l)));
    }
}

// targets come out of the sweep as views; persist them as labels
__global__ void k_view_to_labels(i64 s0, i64 s1,
                                 const unsigned *__restrict__ perm,
                                 const unsigned *__restrict__ vtarget,
                                 const unsigned *__restrict__ sigma, i64 base,
                                 const i64 *__restrict__ rc_ids, i64 lnv,
                                 i64 *__restrict__ out) {
    for (i64 s = s0 + blockIdx.x * (i64)blockDim.x + threadIdx.x; s < s1;
         s += (i64)gridDim.x * blockDim.x) {
        const i64 i = perm[s];
        const unsigned v = vtarget[i];
        out[i] = (v < lnv) ? base + (i64)sigma[v] : rc_ids[v - lnv];
    }
}

// ---- halo #1a delta compaction ----
// The reference resends the FULL ghost community set every iteration
// (dspl.hpp:583-647). Here each export k compares against the label LAST
// SENT and emits a (index-in-segment, label) pair into its peer segment;
// the allgathered count matrix then lets both ends of every pair decide
// full vs compact identically (compact record 12 B vs full 8 B/entry).
// last_sent is updated unconditionally: in full mode the wire carries
// scdata itself, so "last sent" == current either way.
__global__ void k_delta_compact(i64 ssz, const i64 *__restrict__ soff,
                                int nranks, const i64 *__restrict__ scdata,
                                i64 *__restrict__ last_sent,
                                unsigned *__restrict__ chg_idx,
                                i64 *__restrict__ chg_lab,
                                unsigned long long *__restrict__ cnt) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < ssz;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 c = scdata[k];
        if (last_sent[k] == c) continue;
        last_sent[k] = c;
        const int r = (int)dev_lower_bound(soff, nranks + 1, k + 1) - 1;
        const unsigned long long pos = atomicAdd(&cnt[r], 1ull);
        chg_idx[soff[r] + pos] = (unsigned)(k - soff[r]);
        chg_lab[soff[r] + pos] = c;
    }
}

__global__ void k_scatter_deltas(i64 n, const unsigned *__restrict__ idx,
                                 const i64 *__restrict__ lab, i64 seg_base,
                                 i64 *__restrict__ ghost_labels) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x)
        ghost_labels[seg_base + idx[k]] = lab[k];
}

// ---- K8: scdata gather (dspl.hpp:559-571); labels on the wire ----
__global__ void k8_gather_comms(i64 n, const unsigned *__restrict__ svdata_int,
                                const i64 *__restrict__ currComm,
                                i64 *__restrict__ out) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x)
        out[k] = currComm[svdata_int[k]];
}

// ---- candidate remote communities (dspl.hpp:670-700) ----
__global__ void k_filter_remote(i64 n, const i64 *__restrict__ vals,
                                int shift, i64 base, i64 bound,
                                i64 *__restrict__ out,
                                unsigned long long *__restrict__ count) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x) {
        const i64 c = vals[k] >> shift; // label
        if (c < base || c >= bound) out[atomicAdd(count, 1ull)] = c;
    }
}

// per-owner boundaries of a sorted id array (one thread per rank)
__global__ void k_owner_bounds(const i64 *__restrict__ sorted, i64 n,
                               const i64 *__restrict__ parts, int nranks,
                               i64 *__restrict__ bounds) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= nranks) bounds[r] = dev_lower_bound(sorted, n, parts[r]);
}

// ---- K9: cinfo reply gather (dspl.hpp:776-929) ----
__global__ void k9_reply_info(i64 n, const i64 *__restrict__ req_ids, i64 base,
                              const unsigned *__restrict__ sigma_inv,
                              const Cinfo *__restrict__ cinfo,
                              Info16 *__restrict__ out) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x) {
        const Cinfo c = cinfo[sigma_inv[req_ids[k] - base]];
        out[k] = {c.size, c.degree};
    }
}

// apply received deltas to owned cinfo (dspl.hpp:1089-1102; atomics because
// several senders may address one community)
__global__ void k_apply_deltas(i64 n, const i64 *__restrict__ ids, i64 base,
                               const unsigned *__restrict__ sigma_inv,
                               const Info16 *__restrict__ deltas,
                               Cinfo *__restrict__ cinfo) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < n;
         k += (i64)gridDim.x * blockDim.x) {
        Cinfo *c = &cinfo[sigma_inv[ids[k] - base]];
        atomic_add_i64(&c->size, deltas[k].size);
        atomicAdd(&c->degree, deltas[k].degree);
    }
}

// A localCupdate entry nobody moved into or out of is still the all-zero
// bits K6 left there: applying it changes nothing (x + 0 == x, and a sum of
// non-negative degrees is never -0.0) and re-zeroing it rewrites what is there,
// so K6/K67 skip both stores. After the first few iterations that is ~98%
// of the entries, i.e. 32 B/vertex of write traffic per iteration. The test
// is on BITS: a -0.0 degree (deltas that cancelled) is not "clear" and
// takes the full path, so no sign can be left behind.
__device__ __forceinline__ bool cupd_is_clear(const Cinfo &u) {
    return (u.size | __double_as_longlong(u.degree)) == 0;
}

// ---- K6: apply localCupdate (dspl.hpp:458-471), fused with the next
// iteration's K5 zeroing of localCupdate (dspl.hpp:483-484) ----
__global__ void k6_apply_local(i64 lnv, Cinfo *__restrict__ cupd,
                               Cinfo *__restrict__ cinfo) {
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < lnv;
         i += (i64)gridDim.x * blockDim.x) {
        const Cinfo u = cupd[i];
        if (cupd_is_clear(u)) continue; // nothing to apply, nothing to zero
        cinfo[i].size += u.size;
        cinfo[i].degree += u.degree;
        cupd[i] = {0, 0.0};
    }
}

// K6+K7 fused (single-rank path): apply localCupdate, zero it, and emit
// this block's modularity partials in one pass (no remote deltas exist
// between K6 and K7 when nranks == 1)
__global__ void k67_apply_and_partials(i64 lnv, Cinfo *__restrict__ cupd,
                                       Cinfo *__restrict__ cinfo,
                                       const double *__restrict__ cw,
                                       double *__restrict__ out2) {
    double a = 0.0, b = 0.0;
    for (i64 i = blockIdx.x * (i64)blockDim.x + threadIdx.x; i < lnv;
         i += (i64)gridDim.x * blockDim.x) {
        const Cinfo u = cupd[i];
        const i64 nsz = cinfo[i].size + u.size;
        const double nde = cinfo[i].degree + u.degree;
        if (!cupd_is_clear(u)) {
            cinfo[i] = {nsz, nde};
            cupd[i] = {0, 0.0};
        }
        a += cw[i];
        b += nde * nde;
    }
    __shared__ double sa[256], sb[256];
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sa[threadIdx.x] += sa[threadIdx.x + s];
            sb[threadIdx.x] += sb[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out2[2 * blockIdx.x] = sa[0];
        out2[2 * blockIdx.x + 1] = sb[0];
    }
}

// de-permute an internal-ordered label array into original order (trace)
__global__ void k_depermute(i64 lnv, const unsigned *__restrict__ sigma_inv,
                            const i64 *__restrict__ in,
                            i64 *__restrict__ out) {
    for (i64 v = blockIdx.x * (i64)blockDim.x + threadIdx.x; v < lnv;
         v += (i64)gridDim.x * blockDim.x)
        out[v] = in[sigma_inv[v]];
}

// ---- Single-rank (p==1) u32 SLOT community arrays (the encoding is
// described in the K4 note below): init and trace de-permute ----
__global__ void k3_init_comm32(i64 lnv, unsigned *__restrict__ curr,
                               unsigned *__restrict__ past) {
    for (i64 k = blockIdx.x * (i64)blockDim.x + threadIdx.x; k < lnv;
         k += (i64)gridDim.x * blockDim.x) {
        curr[k] = (unsigned)k; // slot k's own community (dspl.hpp:132-149)
        past[k] = (unsigned)k;
    }
}

__global__ void k_depermute32(i64 lnv, const unsigned *__restrict__ sigma,
                              const unsigned *__restrict__ sigma_inv,
                              const unsigned *__restrict__ in,
                              i64 *__restrict__ out) {
    for (i64 v = blockIdx.x * (i64)blockDim.x + threadIdx.x; v < lnv;
         v += (i64)gridDim.x * blockDim.x)
        out[v] = (i64)sigma[in[sigma_inv[v]]]; // slot -> label
}

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
constexpr int QUEUE_HEADS = 8;        // ticket words (one per XCD)
constexpr int QUEUE_HEAD_STRIDE = 16; // u64 between them: a 128-B line each
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
    double *sacc = reinterpret_cast<double *>(smem);
    unsigned *skey =
        reinterpret_cast<unsigned *>(smem + sizeof(double) * SLOTS * B);
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
            int ns = 0, nspill = 0;
            int tb[CH];
            double wb[CH];
            int m = min(CH, deg);
            load_tails<UNIT>(ebase, 0, m, sell_tidx, sell_w, tb, wb);
            const Cinfo cci = comm_info<MR>(cc, lnv, cinfo, rc_info);
            for (int k0 = 0;;) {
                unsigned cb[CH];
                gather_comms<MR>(tb, lnv, vcurr, vghost, cb);
                for (int j = 0; j < m; j++) {
                    const i64 tidx = tb[j];
                    const double w = UNIT ? 1.0 : wb[j];
                    if (tidx == i) selfLoop += w; // dspl.hpp:247-248
                    const unsigned tcomm = cb[j];
                    if (tcomm == cc) { c0 += w; continue; }
                    bool found = false;
                    for (int t = 0; t < ns; t++) {
                        if (skey[t * B + tid] == tcomm) {
                            sacc[t * B + tid] += w;
                            found = true;
                            break;
                        }
                    }
                    if (found) continue;
                    if (ns < SLOTS) {
                        skey[ns * B + tid] = tcomm;
                        sacc[ns * B + tid] = w;
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
            for (int t = 0; t < ns; t++)
                argmax_step<MR>(skey[t * B + tid], sacc[t * B + tid], eix,
                                vdeg, ax, constant, lnv, base, sigma, cinfo,
                                rc_ids, rc_info, maxGain, maxIndex, maxSize);
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

int grid_for(i64 n, int block = 256, int cap = 2048) {
    i64 g = (n + block - 1) / block;
    return (int)std::min<i64>(std::max<i64>(g, 1), cap);
}

// Move-only owner of one device (hipMalloc) or pinned host (hipHostMalloc)
// allocation. reserve() is grow-only and does NOT preserve contents; it
// floors n at one element so the pointer is never null once reserved.
template <class T, bool PINNED = false> struct DevBuf {
    T *ptr = nullptr;
    i64 cap = 0; // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), cap(o.cap) {
        o.ptr = nullptr;
        o.cap = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(ptr, o.ptr); // o's destructor frees what we held
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { release(); }
    // true when it (re)allocated
    bool reserve(i64 n) {
        n = std::max<i64>(n, 1);
        if (n <= cap) return false;
        release();
        if (PINNED)
            HIP_CHECK(hipHostMalloc((void **)&ptr, sizeof(T) * n));
        else
            HIP_CHECK(hipMalloc((void **)&ptr, sizeof(T) * n));
        cap = n;
        return true;
    }
    void release() {
        if (!ptr) return;
        if (PINNED)
            HIP_CHECK(hipHostFree(ptr));
        else
            HIP_CHECK(hipFree(ptr));
        ptr = nullptr;
        cap = 0;
    }
    // take over a device allocation of n >= 1 elements made elsewhere
    // with hipMalloc (what was held is freed); the caller lets go of p
    void adopt(T *p, i64 n) {
        static_assert(!PINNED, "adopt() takes hipMalloc memory");
        release();
        ptr = p;
        cap = n;
    }
    T *get() const { return ptr; }
    operator T *() const { return ptr; }
};
template <class T> using PinBuf = DevBuf<T, true>;

// one point-to-point message of a batched exchange (see exchange())
struct Xfer {
    int peer;
    void *ptr;
    ncclDataType_t ty;
    i64 count; // elements of ty
};

} // namespace

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
    int sort_bits = 64; // ceil(log2(nv)): radix sort width for id keys
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

static void build_sell(mv_engine *e);

// free everything a previous load_graph/run allocated (engines may be
// re-pointed at a new graph). The caller has set the device.
static void free_graph_state(mv_engine *e) {
    // this also clears trace_target / trace_mod / trace_cap: a stale trace
    // against a freed d_trace_tmp (or a new lnv) would fault, so re-arm via
    // mv_engine_set_trace after every load
    static_cast<mv_graph_state &>(*e) = mv_graph_state{};
}

// the part both constructors share: device check, streams and events
static mv_engine *engine_new(const char *who, int device, int rank,
                             int nranks) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
        std::fprintf(stderr,
                     "%s: no HIP device %d (found %d). The MI355X engine "
                     "has no CPU fallback.\n",
                     who, device, ndev);
        return nullptr;
    }
    auto *e = new mv_engine;
    e->device = device;
    e->rank = rank;
    e->nranks = nranks;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipDeviceGetAttribute(&e->num_cus,
                                    hipDeviceAttributeMultiprocessorCount,
                                    device));
    HIP_CHECK(hipStreamCreate(&e->stream));
    HIP_CHECK(hipStreamCreate(&e->stream2));
    HIP_CHECK(hipEventCreate(&e->ev_p1));
    HIP_CHECK(hipEventCreate(&e->ev_p2));
    HIP_CHECK(hipEventCreate(&e->ev_cinfo));
    HIP_CHECK(hipEventCreate(&e->ev_halo));
    return e;
}

extern "C" {

int mv_comm_id(void *id_bytes) {
    static_assert(sizeof(ncclUniqueId) <= MV_COMM_ID_BYTES, "id size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
    std::memcpy(id_bytes, &id, sizeof(id));
    return 0;
}

mv_engine *mv_engine_create(int device, int rank, int nranks,
                            const void *comm_id) {
    if (nranks > 1 && !comm_id) {
        std::fprintf(stderr, "mv_engine_create: nranks>1 needs comm id\n");
        return nullptr;
    }
    mv_engine *e = engine_new("mv_engine_create", device, rank, nranks);
    if (e && nranks > 1) {
        ncclUniqueId id;
        std::memcpy(&id, comm_id, sizeof(id));
        NCCL_CHECK(ncclCommInitRank(&e->comm, nranks, id, rank));
        // halo #1a rides its own communicator so RCCL can run it
        // concurrently with the epilogue's collectives (MV_NO_OVERLAP must
        // be set on ALL ranks or none — ncclCommSplit is collective)
        if (!getenv("MV_NO_OVERLAP"))
            NCCL_CHECK(ncclCommSplit(e->comm, 0, rank, &e->comm2, nullptr));
    }
    return e;
}

mv_lb_session *mv_lb_create(int nranks) { return new mv_lb_session(nranks); }

void mv_lb_destroy(mv_lb_session *s) { delete s; }

mv_engine *mv_engine_create_lb(int device, int rank, int nranks,
                               mv_lb_session *s) {
    if (!s || s->nranks != nranks) {
        std::fprintf(stderr, "mv_engine_create_lb: bad session\n");
        return nullptr;
    }
    mv_engine *e = engine_new("mv_engine_create_lb", device, rank, nranks);
    if (e) e->lb = s;
    return e;
}

void mv_engine_destroy(mv_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device); // teardown: best effort
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->ev_p1) (void)hipEventDestroy(e->ev_p1);
    if (e->ev_p2) (void)hipEventDestroy(e->ev_p2);
    if (e->ev_cinfo) (void)hipEventDestroy(e->ev_cinfo);
    if (e->ev_halo) (void)hipEventDestroy(e->ev_halo);
    if (e->comm2) ncclCommDestroy(e->comm2);
    if (e->comm) ncclCommDestroy(e->comm);
    free_graph_state(e);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// Default window (vertices; 0 = off) and degree quantum of the windowed
// degree order: the best pair measured on the bench workload
// (experiments/RESULTS.md, "windowed degree order").
constexpr i64 DEG_WINDOW_DEFAULT = 2048;
constexpr i64 DEG_QUANT_DEFAULT = 4;

// Decide the windowed degree order of this graph (mv_sweep_info documents
// the rule): needs has_hint, skewed, lnv and sweep_grid. MV_DEG_WINDOW /
// MV_DEG_QUANT are read at every load (perf only, results identical).
static void choose_degree_windows(mv_engine *e) {
    e->deg_window = 0;
    e->deg_quant = 1;
    e->row_group = 1;
    if (!e->has_hint || e->skewed) return;
    const char *ws = getenv("MV_DEG_WINDOW");
    const char *qs = getenv("MV_DEG_QUANT");
    const i64 W = ws ? atoll(ws) : DEG_WINDOW_DEFAULT;
    const i64 q = qs ? atoll(qs) : DEG_QUANT_DEFAULT;
    if (W <= 0) return;
    if (W < 128 || (W & (W - 1)) || q < 1) {
        std::fprintf(stderr, "MV_DEG_WINDOW must be 0 or a power of two >= "
                             "128 and MV_DEG_QUANT >= 1: degree windows off\n");
        return;
    }
    i64 S = 1;
    if (ws) { // an explicit window is honoured even where waves then idle
        S = std::min<i64>(W / 64, 8);
    } else {
        const i64 rows = (e->lnv + 63) / 64;
        const i64 waves = 4 * (i64)e->sweep_grid;
        const i64 cap = std::min(W / 64, (rows + waves - 1) / waves);
        while (S * 2 <= cap) S *= 2;
        if (S < 2) return; // a row per wave at most: keep every wave busy
    }
    e->deg_window = W;
    e->deg_quant = q;
    e->row_group = (int)S;
}

// Largest default queue unit (rows) of the general sweep: the best cell of
// the measured U x grid table (experiments/RESULTS.md, "row queue").
constexpr int SWEEP_UNIT_DEFAULT = 4;

// Decide the row queue of this graph's general sweeps and the grid cap
// (mv_sweep_info documents both). Runs after choose_degree_windows, which
// keeps seeing the uncapped grid: the layout rule does not depend on these
// knobs. MV_SWEEP_UNIT / MV_SWEEP_GRID / MV_SWEEP_QUEUE_FROM are read at
// every load (perf only, results identical).
static void choose_row_queue(mv_engine *e) {
    const char *us = getenv("MV_SWEEP_UNIT");
    const char *gs = getenv("MV_SWEEP_GRID");
    const int cap = gs ? atoi(gs) : 0;
    if (cap > 0) e->sweep_grid = std::min(e->sweep_grid, cap);
    int U = 0;
    if (us) { // an explicit unit is honoured even where waves then idle
        U = atoi(us);
        if (U < 0 || U > 4096) {
            std::fprintf(stderr, "MV_SWEEP_UNIT must be in [0, 4096]: "
                                 "static row schedule\n");
            U = 0;
        }
    } else { // at least two units per wave, or the queue has nothing to do
        const i64 rows = (e->lnv + 63) / 64;
        const i64 per_wave = rows / (4 * (i64)e->sweep_grid);
        for (U = SWEEP_UNIT_DEFAULT; U > 2 && 2 * U > per_wave; U /= 2) {}
        if (2 * U > per_wave) U = 0;
    }
    // skewed graphs size each thread's spill from the vertices the static
    // schedule hands it (k_spill_need): only uniform extents let any
    // thread take any vertex
    e->sched_unit = e->skewed ? 0 : U;
    const char *fs = getenv("MV_SWEEP_QUEUE_FROM");
    e->sched_from = fs ? std::max(atoi(fs), 0) : 0;
    e->sched_grid = 0;
    for (auto &t : e->tickets_total) t = 0;
    e->d_ticket.reserve(QUEUE_HEADS * QUEUE_HEAD_STRIDE);
    HIP_CHECK(hipMemset(e->d_ticket, 0,
                        8 * QUEUE_HEADS * QUEUE_HEAD_STRIDE));
}

int mv_engine_load_graph(mv_engine *e, const mv_graph *g) {
    HIP_CHECK(hipSetDevice(e->device));
    if (e->d_xadj) free_graph_state(e); // re-load on a live engine
    e->nv = mv_graph_nv(g);
    if (e->nv >= (1ll << 31)) { // u32 slot/view encodings + int32 SELL
                                // tails need 31-bit ids
        std::fprintf(stderr, "mv_engine_load_graph: nv >= 2^31 unsupported\n");
        return -1;
    }
    e->lnv = mv_graph_lnv(g);
    e->lne = mv_graph_lne(g);
    e->sort_bits = 1;
    while ((1ll << e->sort_bits) < e->nv) e->sort_bits++;
    e->parts_h.assign(mv_graph_parts(g), mv_graph_parts(g) + e->nranks + 1);
    e->base = e->parts_h[e->rank];
    e->bound = e->parts_h[e->rank + 1];
    const i64 lnv = e->lnv, lne = e->lne;

    const i64 *xadj = mv_graph_xadj(g);
    e->max_degree = 0;
    for (i64 i = 0; i < lnv; i++)
        e->max_degree = std::max(e->max_degree, xadj[i + 1] - xadj[i]);
    const double *w = mv_graph_weights(g);
    e->unit_weights = 1;
    for (i64 k = 0; k < lne; k++)
        if (w[k] != 1.0) { e->unit_weights = 0; break; }
    const i64 *tails_h = mv_graph_tails(g);
    e->rows_sorted = 1;
    for (i64 i = 0; i < lnv && e->rows_sorted; i++)
        for (i64 k = xadj[i] + 1; k < xadj[i + 1]; k++)
            if (tails_h[k - 1] > tails_h[k]) { e->rows_sorted = 0; break; }

    e->d_parts.reserve(e->nranks + 1);
    HIP_CHECK(hipMemcpy(e->d_parts, e->parts_h.data(), 8 * (e->nranks + 1),
                        hipMemcpyHostToDevice));
    e->d_xadj.reserve(lnv + 1);
    HIP_CHECK(hipMemcpy(e->d_xadj, xadj, 8 * (lnv + 1), hipMemcpyHostToDevice));
    e->d_tails.reserve(lne);
    if (lne) // an empty slice's vectors may hand out null data()
        HIP_CHECK(hipMemcpy(e->d_tails, mv_graph_tails(g), 8 * lne,
                            hipMemcpyHostToDevice));
    // unit graphs never read edge weights on device (K1 counts rows, the
    // SELL carries no weight stream): skip the 8*lne upload entirely
    if (e->unit_weights) {
        e->d_ew.reserve(2); // never-null dummy
    } else {
        e->d_ew.reserve(lne);
        HIP_CHECK(hipMemcpy(e->d_ew, w, 8 * lne, hipMemcpyHostToDevice));
    }

    // internal layout: the builder's spatial hint, or identity (the
    // degree-sort fallback then runs in the per-run setup)
    e->d_sigma.reserve(lnv);
    e->d_sigma_inv.reserve(lnv);
    const int32_t *hint = mv_graph_locality_hint(g);
    e->has_hint = hint != nullptr;
    // K4 geometry first: the windowed degree order depends on it
    e->sweep_grid = grid_for(lnv, 256, 2048);
    e->skewed = e->max_degree > 256;
    choose_degree_windows(e);
    choose_row_queue(e);
    if (hint && e->deg_window) {
        // uniform-degree SELL slices: refine the hint inside its spatial
        // windows (mv_degree_window_order). sigma carries it, so perm stays
        // the identity and every per-vertex array stays coalesced.
        std::vector<int32_t> refined(lnv);
        if (mv_degree_window_order(hint, xadj, lnv, e->deg_window,
                                   e->deg_quant, e->row_group,
                                   refined.data()) != 0) {
            std::fprintf(stderr, "mv_engine_load_graph: bad degree window\n");
            return -1;
        }
        HIP_CHECK(hipMemcpy(e->d_sigma, refined.data(), 4 * lnv,
                            hipMemcpyHostToDevice));
    } else if (hint) {
        HIP_CHECK(hipMemcpy(e->d_sigma, hint, 4 * lnv, hipMemcpyHostToDevice));
    } else {
        k_iota32<<<grid_for(lnv), 256>>>(lnv, e->d_sigma);
    }
    k_invert_perm<<<grid_for(lnv), 256>>>(lnv, e->d_sigma, e->d_sigma_inv);

    e->nchunks = (lnv + 63) / 64;
    e->d_deg.reserve(lnv);
    e->d_iota.reserve(lnv);
    e->d_perm.reserve(lnv);
    e->d_chunk_off.reserve(e->nchunks + 1);

    e->d_curr.reserve(lnv);
    e->d_past.reserve(lnv);
    e->d_target.reserve(lnv);
    e->d_vdeg.reserve(lnv);
    e->d_cw.reserve(lnv);
    e->d_cinfo.reserve(lnv);
    e->d_cupd.reserve(lnv);
    // never-null dummies for pointers that stay unused at nranks==1 but
    // may still be address-computed by if-converted loads
    e->d_vghost.reserve(4);
    e->d_rc_ids.reserve(2);
    e->d_rc_info.reserve(1);
    e->d_rcu.reserve(1);
    e->d_count.reserve(1);
    e->d_bounds.reserve(e->nranks + 1);
    e->d_red.reserve(3);
    const int nblocks = grid_for(lnv);
    e->d_partials.reserve(2 * nblocks);
    e->h_partials.reserve(2 * nblocks);

    // K4 geometry: 256-thread blocks, 8 LDS slots/lane (32 KiB/block ->
    // 4-5 blocks/CU). Spill sizing: uniform per-thread max_degree extents
    // for flat distributions; for skewed graphs (max degree > 256) the
    // SELL order is forced degree-descending and extents follow the
    // per-thread first-vertex degree (k_spill_need), so the total stays
    // O(lne) instead of O(threads * max_degree).
    const i64 nthreads = (i64)e->sweep_grid * 256;
    e->d_spill_off.reserve(nthreads);

    if (e->nranks == 1) build_sell(e);
    HIP_CHECK(hipDeviceSynchronize());
    e->stats = mv_stats{};
    e->sweep = mv_sweep_info{};
    e->halo = mv_halo_info{};
    e->stats.edges_local = lne;
    return 0;
}

void mv_engine_set_trace(mv_engine *e, int64_t *target_trace, double *mod_trace,
                         int cap) {
    e->trace_target = target_trace;
    e->trace_mod = mod_trace;
    e->trace_cap = cap;
    if (target_trace) e->d_trace_tmp.reserve(e->lnv);
}

void mv_engine_get_stats(const mv_engine *e, mv_stats *out) { *out = e->stats; }

void mv_engine_get_sweep_info(const mv_engine *e, mv_sweep_info *out) {
    *out = e->sweep; // the launch counters of the last run
    out->nhi = e->nhi;
    out->nlh = e->nlh;
    out->nghost = e->nghost;
    out->ssz = e->ssz;
    out->nexp = e->nexp;
    out->skewed = e->skewed;
    out->overlap = e->overlap;
    out->rows_sorted = e->rows_sorted;
    out->sell_sorted = e->sell_sorted;
    out->unit_weights = e->unit_weights;
    out->deg_window = e->deg_window;
    out->deg_quant = e->deg_quant;
    out->row_group = e->row_group;
    out->sell_entries = e->sell_entries;
    out->sched_unit = e->sched_unit;
    out->sched_grid = e->sched_grid;
    out->perm_identity = e->perm_identity;
    out->sched_tickets_expected = 0;
    for (auto t : e->tickets_total) out->sched_tickets_expected += (int64_t)t;
    out->sched_tickets = 0;
    // the device words, read now (after the run's work): the one part of
    // this call that touches the device, and only with the queue on
    if (e->sched_unit && e->d_ticket) {
        unsigned long long t[QUEUE_HEADS];
        HIP_CHECK(hipSetDevice(e->device));
        HIP_CHECK(hipStreamSynchronize(e->stream));
        HIP_CHECK(hipMemcpy2D(t, 8, e->d_ticket, 8 * QUEUE_HEAD_STRIDE, 8,
                              QUEUE_HEADS, hipMemcpyDeviceToHost));
        for (auto v : t) out->sched_tickets += (int64_t)v;
    }
}

void mv_engine_get_halo_info(const mv_engine *e, mv_halo_info *out) {
    *out = e->halo;
}

// ------------------------------------------------------------------------
// Transport seam. Three primitives — exchange(), allgather_counts() and
// comm_allreduce_host() — each with an RCCL arm (the product path) and a
// loopback arm (device-to-device copies + host barriers). The protocol code
// that calls them builds ONE plan per exchange and never asks which arm runs.

static bool has_second_channel(const mv_engine *e) {
    return e->comm2 || e->lb; // loopback needs no second communicator
}

static size_t ty_bytes(ncclDataType_t ty) {
    if (ty == ncclChar) return 1;
    if (ty == ncclInt64) return 8;
    std::fprintf(stderr, "exchange: unsupported datatype %d\n", (int)ty);
    std::abort();
}

// Batched point-to-point exchange. Both lists ascend by peer and may hold
// several entries per peer; the k-th send of rank a to rank b lands in
// b's k-th recv from a. RCCL: one group, peer by peer, a peer's sends then
// its recvs. Loopback: each rank pulls the sends addressed to it.
static void exchange(mv_engine *e, const std::vector<Xfer> &sends,
                     const std::vector<Xfer> &recvs, ncclComm_t comm,
                     hipStream_t stream) {
    const int p = e->nranks, me = e->rank;
    if (e->lb) {
        mv_lb_session *s = e->lb;
        // own kernels feeding the sends must be complete before peers copy
        HIP_CHECK(hipStreamSynchronize(stream));
        s->posts[me].sends = &sends;
        s->barrier();
        size_t j = 0;
        for (int r = 0; r < p; r++) {
            if (r == me) continue;
            for (const Xfer &x : *s->posts[r].sends) {
                if (x.peer != me) continue;
                const bool have = j < recvs.size() && recvs[j].peer == r;
                const size_t sb = x.count * ty_bytes(x.ty);
                const size_t rb =
                    have ? recvs[j].count * ty_bytes(recvs[j].ty) : 0;
                if (!have || sb != rb) {
                    std::fprintf(stderr,
                                 "loopback exchange mismatch: me=%d r=%d "
                                 "sender says %zu bytes, I expect %zu\n",
                                 me, r, sb, rb);
                    std::abort();
                }
                HIP_CHECK(hipMemcpyAsync(recvs[j++].ptr, x.ptr, sb,
                                         hipMemcpyDeviceToDevice, stream));
            }
            if (j < recvs.size() && recvs[j].peer == r) {
                std::fprintf(stderr,
                             "loopback exchange mismatch: me=%d r=%d sent "
                             "fewer messages than I expect\n",
                             me, r);
                std::abort();
            }
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        s->barrier(); // senders may reuse their buffers after this
        return;
    }
    NCCL_CHECK(ncclGroupStart());
    size_t i = 0, j = 0;
    for (int r = 0; r < p; r++) {
        for (; i < sends.size() && sends[i].peer == r; i++)
            NCCL_CHECK(ncclSend(sends[i].ptr, sends[i].count, sends[i].ty, r,
                                comm, stream));
        for (; j < recvs.size() && recvs[j].peer == r; j++)
            NCCL_CHECK(ncclRecv(recvs[j].ptr, recvs[j].count, recvs[j].ty, r,
                                comm, stream));
    }
    NCCL_CHECK(ncclGroupEnd());
}

// alltoallv over exchange(); offsets in elements of elem_bytes, sent as
// `ty`. Empty segments are skipped.
static void alltoallv(mv_engine *e, const void *send, const i64 *soff,
                      void *recv, const i64 *roff, size_t elem_bytes,
                      ncclDataType_t ty, ncclComm_t comm, hipStream_t stream) {
    const i64 per = (i64)(elem_bytes / ty_bytes(ty));
    std::vector<Xfer> sends, recvs;
    for (int r = 0; r < e->nranks; r++) {
        if (r == e->rank) continue;
        const i64 scnt = soff[r + 1] - soff[r];
        const i64 rcnt = roff[r + 1] - roff[r];
        if (scnt > 0)
            sends.push_back({r, (char *)send + soff[r] * elem_bytes, ty,
                             scnt * per});
        if (rcnt > 0)
            recvs.push_back({r, (char *)recv + roff[r] * elem_bytes, ty,
                             rcnt * per});
    }
    exchange(e, sends, recvs, comm, stream);
}

// Count allgather: my nranks counts (`mine`, on the host or on the device)
// -> every rank's row in the host matrix (nranks*nranks). Returns with the
// matrix complete.
static void allgather_counts(mv_engine *e, const i64 *mine, bool on_device,
                             i64 *matrix, ncclComm_t comm,
                             hipStream_t stream) {
    const int p = e->nranks;
    if (e->lb) {
        mv_lb_session *s = e->lb;
        std::vector<int64_t> &post = s->posts[e->rank].cnts;
        post.resize(p);
        if (on_device) {
            HIP_CHECK(hipMemcpyAsync(post.data(), mine, 8 * p,
                                     hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        } else {
            std::copy(mine, mine + p, post.begin());
        }
        s->barrier();
        for (int r = 0; r < p; r++)
            std::copy(s->posts[r].cnts.begin(), s->posts[r].cnts.end(),
                      matrix + (size_t)r * p);
        s->barrier();
        return;
    }
    // persistent buffer (allocated by the first, setup-time call): a
    // hipMalloc/hipFree here would device-sync and re-serialize the
    // overlapped pipeline. One matrix serves every caller: each call
    // returns only after its D2H copy has synced, and a rank issues its
    // allgathers from one host thread.
    e->d_cntmat.reserve((i64)p * p);
    i64 *d_all = e->d_cntmat, *row = d_all + (i64)e->rank * p;
    HIP_CHECK(hipMemcpyAsync(row, mine, 8 * p,
                             on_device ? hipMemcpyDeviceToDevice
                                       : hipMemcpyHostToDevice,
                             stream));
    NCCL_CHECK(ncclAllGather(row, d_all, p, ncclInt64, comm, stream));
    HIP_CHECK(hipMemcpyAsync(matrix, d_all, 8 * p * p, hipMemcpyDeviceToHost,
                             stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// allreduce-sum of n (<= 3) host doubles in place (dspl.hpp:126, :441)
static void comm_allreduce_host(mv_engine *e, double *vals, int n) {
    if (e->lb) {
        mv_lb_session *s = e->lb;
        s->posts[e->rank].red = vals;
        s->barrier();
        double acc[3] = {0.0, 0.0, 0.0};
        for (int r = 0; r < e->nranks; r++) // rank order: deterministic
            for (int k = 0; k < n; k++) acc[k] += s->posts[r].red[k];
        s->barrier(); // all ranks have read every post
        for (int k = 0; k < n; k++) vals[k] = acc[k];
        return;
    }
    e->d_red.reserve(3); // a level's q is reduced before the first load
    HIP_CHECK(hipMemcpyAsync(e->d_red, vals, 8 * n, hipMemcpyHostToDevice,
                             e->stream));
    NCCL_CHECK(ncclAllReduce(e->d_red, e->d_red, n, ncclDouble, ncclSum,
                             e->comm, e->stream));
    HIP_CHECK(hipMemcpyAsync(vals, e->d_red, 8 * n, hipMemcpyDeviceToHost,
                             e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
}

// Build the SELL image, internal order, spill extents and the high-degree
// hash regions. Pure graph-layout preparation (a function of the static
// graph + the ghost list), analogous to the reference's CSR existing
// before its timed span; called at load for single-rank graphs and right
// after ghost discovery inside the span for multi-rank ones (the ghost
// slots feed the tail translation).
static void build_sell(mv_engine *e) {
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv;
    // build the SELL image over the internal order (tails translated
    // inline). perm = identity with a spatial hint, degree-sorted
    // otherwise (load balance for skewed degree distributions).
    k_degrees<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_sigma, e->d_xadj,
                                             e->d_deg);
    e->nhi = 0; // set by the skewed branch below when applicable
    e->nlh = 0;
    e->perm_identity = 0;
    if (e->has_hint && !e->skewed) {
        k_iota32<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_perm);
        e->perm_identity = 1; // until something below permutes it
    } else {
        k_iota32<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_iota);
        DevBuf<unsigned> d_degs; // temporaries: freed with this block
        DevBuf<char> d_tmp;
        d_degs.reserve(lnv);
        size_t tb = 0;
        (void)hipcub::DeviceRadixSort::SortPairsDescending(
            nullptr, tb, e->d_deg.get(), d_degs.get(), e->d_iota.get(),
            e->d_perm.get(), lnv, 0, 32, st);
        d_tmp.reserve(tb);
        (void)hipcub::DeviceRadixSort::SortPairsDescending(
            d_tmp.get(), tb, e->d_deg.get(), d_degs.get(), e->d_iota.get(),
            e->d_perm.get(), lnv, 0, 32, st);
        // high-degree split + per-vertex hash regions (unit: wave-per-
        // vertex atomic hash; -w: per-lane serial hash in edge order)
        std::vector<unsigned> sdeg(lnv);
        if (lnv) // a rank may own no vertices (null data())
            HIP_CHECK(hipMemcpyAsync(sdeg.data(), d_degs, 4 * lnv,
                                     hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        // MV_HI_THRESH (perf only): degree bound above which a vertex
        // takes the hub path (wave hash for unit, per-lane hash for -w)
        // instead of the LDS-slot + linear-spill lane path
        static const unsigned HI_THRESH = [] {
            const char *s = getenv("MV_HI_THRESH");
            return s ? (unsigned)atoi(s) : 256u;
        }();
        // MV_LH_THRESH: degree bound above which a vertex takes the
        // per-lane hash band (below: LDS slots + linear spill). Default ==
        // HI_THRESH: the band only covers WEIGHTED hubs (where it replaces
        // the old cap-scanning kernel); extending it to the unit 24-256
        // band was measured SLOWER than 24 LDS slots + linear spill on the
        // dense social shape (11.3 -> 8.3 G, experiments/RESULTS.md) — L2
        // hash probes lose to LDS at ~25 candidates.
        static const unsigned LH_THRESH = [] {
            const char *s = getenv("MV_LH_THRESH");
            return s ? (unsigned)atoi(s) : 256u;
        }();
        i64 nhi = 0;
        while (nhi < lnv && sdeg[nhi] > HI_THRESH) nhi++;
        i64 nlh = 0;
        while (nlh < lnv && sdeg[nlh] > LH_THRESH) nlh++;
        e->nhi = (e->skewed && e->unit_weights) ? nhi : 0;
        e->nlh = e->skewed ? std::max<i64>(nlh, e->nhi) : 0;
        if (e->nlh > 0) {
            e->d_tidx32.reserve(e->lne);
            k_translate_tails<<<grid_for(e->lne), 256, 0, st>>>(
                e->lne, e->d_tails, e->base, e->bound, e->d_sigma_inv,
                e->d_ghosts, e->nghost, lnv, e->d_tidx32);
            std::vector<i64> hoff(e->nlh + 1);
            i64 acc = 0;
            for (i64 t = 0; t < e->nlh; t++) {
                hoff[t] = acc;
                i64 cap = 64;
                while (cap < 2 * (i64)sdeg[t]) cap <<= 1;
                acc += cap;
            }
            hoff[e->nlh] = acc;
            e->hash_hub_elems = e->nhi > 0 ? hoff[e->nhi] : 0;
            e->d_hash_off.reserve(e->nlh + 1);
            HIP_CHECK(hipMemcpyAsync(e->d_hash_off, hoff.data(),
                                     8 * (e->nlh + 1),
                                     hipMemcpyHostToDevice, st));
            e->hash_total = acc;
            if (e->d_hkeys.reserve(acc)) { // the three grow together
                e->d_hacc.reserve(acc);
                e->d_lh_list.reserve(acc / 2 + 1);
            }
            HIP_CHECK(hipStreamSynchronize(st));
        }
    }

    // Exports-first SELL order (halo overlap): positions [0, nexp) hold
    // the vertices some peer wants (the svdata set), so the sweep can run
    // them as a first launch and halo #1a for the NEXT iteration — which
    // only needs their targets — can overlap the interior sweep + the
    // whole epilogue on stream2/comm2 (north_star: "#1a overlapped with
    // the local sweep on a second HIP stream"). Stable partition: locality
    // inside each group is preserved. Pure layout, results identical.
    e->nexp = 0;
    e->overlap = 0;
    if (e->nranks > 1 && !e->skewed && e->ssz > 0 && has_second_channel(e) &&
        !getenv("MV_NO_OVERLAP")) {
        // device-side stable partition (two hipCUB Flagged selects): the
        // host round trip cost ~ms per run at 8-GPU sizes
        DevBuf<unsigned char> d_mark, d_flags; // freed with this block
        DevBuf<unsigned> d_out;
        DevBuf<i64> d_num;
        DevBuf<char> d_tsel;
        d_mark.reserve(lnv);
        d_flags.reserve(lnv);
        d_out.reserve(lnv);
        d_num.reserve(1);
        HIP_CHECK(hipMemsetAsync(d_mark, 0, lnv, st));
        k_scatter_mark<<<grid_for(e->ssz), 256, 0, st>>>(
            e->ssz, e->d_svdata_int, d_mark);
        k_gather_flags<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_perm, d_mark,
                                                      d_flags, 0);
        size_t tsel = 0;
        (void)hipcub::DeviceSelect::Flagged(nullptr, tsel, e->d_perm.get(),
                                            d_flags.get(), d_out.get(),
                                            d_num.get(), lnv, st);
        d_tsel.reserve(tsel);
        (void)hipcub::DeviceSelect::Flagged(d_tsel.get(), tsel,
                                            e->d_perm.get(), d_flags.get(),
                                            d_out.get(), d_num.get(), lnv, st);
        HIP_CHECK(hipMemcpyAsync(&e->nexp, d_num, 8, hipMemcpyDeviceToHost,
                                 st));
        HIP_CHECK(hipStreamSynchronize(st));
        k_gather_flags<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_perm, d_mark,
                                                      d_flags, 1);
        (void)hipcub::DeviceSelect::Flagged(d_tsel.get(), tsel,
                                            e->d_perm.get(), d_flags.get(),
                                            d_out + e->nexp, d_num.get(), lnv,
                                            st);
        HIP_CHECK(hipMemcpyAsync(e->d_perm, d_out, 4 * lnv,
                                 hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        e->overlap = 1;
        e->perm_identity = 0;
    }

    {
        DevBuf<i64> d_sizes; // freed with this block
        DevBuf<char> d_tmp2;
        d_sizes.reserve(e->nchunks);
        k_chunk_sizes<<<grid_for(e->nchunks), 256, 0, st>>>(
            e->nchunks, lnv, e->d_perm, e->d_deg, d_sizes);
        HIP_CHECK(hipMemsetAsync(e->d_chunk_off, 0, 8, st));
        size_t tb2 = 0;
        (void)hipcub::DeviceScan::InclusiveSum(nullptr, tb2, d_sizes.get(),
                                         e->d_chunk_off + 1, e->nchunks,
                                         st);
        d_tmp2.reserve(tb2);
        (void)hipcub::DeviceScan::InclusiveSum(d_tmp2.get(), tb2,
                                         d_sizes.get(), e->d_chunk_off + 1,
                                         e->nchunks, st);
        i64 total = 0;
        HIP_CHECK(hipMemcpyAsync(&total, e->d_chunk_off + e->nchunks, 8,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        e->sell_entries = total;
        e->d_sell_tidx.reserve(total);
        if (!e->unit_weights) e->d_sell_w.reserve(total);
        k_fill_sell<<<grid_for(lnv), 256, 0, st>>>(
            lnv, e->d_perm, e->d_sigma, e->d_sigma_inv, e->d_xadj,
            e->d_tails, e->d_ew, e->base, e->bound, e->d_ghosts, e->nghost,
            e->d_chunk_off, e->d_sell_tidx,
            e->unit_weights ? nullptr : e->d_sell_w.get());
        // unit graphs: re-sort rows by internal index for gather locality
        // (see k_sell_sort_rows; results identical, measured +4-5%)
        e->sell_sorted = 0;
        if (e->unit_weights && !e->skewed && !getenv("MV_NO_ROWSORT")) {
            k_sell_sort_rows<<<grid_for(lnv), 256, 0, st>>>(
                lnv, e->d_perm, e->d_deg, e->d_chunk_off, e->d_sell_tidx);
            e->sell_sorted = 1;
        }
    }

    // per-thread spill extents
    {
        const i64 nthreads = (i64)e->sweep_grid * 256;
        i64 total;
        if (!e->skewed) {
            const i64 per = std::max<i64>(e->max_degree, 1);
            k_spill_uniform<<<grid_for(nthreads), 256, 0, st>>>(
                nthreads, per, e->d_spill_off);
            total = nthreads * per;
        } else {
            DevBuf<i64> d_need; // freed with this block
            d_need.reserve(nthreads);
            k_spill_need<<<grid_for(nthreads), 256, 0, st>>>(
                nthreads, e->nlh, lnv, e->d_perm, e->d_deg, 4, d_need);
            std::vector<i64> need(nthreads), off(nthreads);
            HIP_CHECK(hipMemcpyAsync(need.data(), d_need, 8 * nthreads,
                                     hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            i64 acc = 0;
            for (i64 t = 0; t < nthreads; t++) {
                off[t] = acc;
                acc += need[t];
            }
            total = acc;
            HIP_CHECK(hipMemcpyAsync(e->d_spill_off, off.data(),
                                     8 * nthreads, hipMemcpyHostToDevice,
                                     st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        e->d_spill_k.reserve(total);
        e->d_spill_a.reserve(total);
    }

    HIP_CHECK(hipStreamSynchronize(st));
}

// Halo #1a (dspl.hpp:583-647) on (comm, stream): gather the exports'
// communities, exchange them (full resend like the reference, or
// delta-compacted), and scatter into the persistent label image
// d_ghost_labels (the per-iteration u32 view is built from it once the
// rc set is known). In overlap mode this runs on stream2/comm2
// concurrently with the interior sweep + epilogue.
static void run_halo1a(mv_engine *e, const i64 *commArr, ncclComm_t comm,
                       hipStream_t st2) {
    const int p = e->nranks;
    e->halo.exchanges++;
    k8_gather_comms<<<grid_for(std::max<i64>(e->ssz, 1)), 256, 0, st2>>>(
        e->ssz, e->d_svdata_int, commArr, e->d_scdata);
    if (!e->use_delta) {
        for (int r = 0; r < p; r++) { // every non-empty segment goes whole
            if (r == e->rank) continue;
            if (e->send_off[r + 1] > e->send_off[r]) e->halo.send_full++;
            if (e->recv_off[r + 1] > e->recv_off[r]) e->halo.recv_full++;
        }
        alltoallv(e, e->d_scdata, e->send_off.data(), e->d_ghost_labels,
                  e->recv_off.data(), 8, ncclInt64, comm, st2);
    } else {
        HIP_CHECK(hipMemsetAsync(e->d_chg_cnt, 0, 8 * p, st2));
        k_delta_compact<<<grid_for(std::max<i64>(e->ssz, 1)), 256, 0, st2>>>(
            e->ssz, e->d_soff, p, e->d_scdata, e->d_last_sent, e->d_chg_idx,
            e->d_chg_lab, e->d_chg_cnt);
        // tiny count matrix; rides the same stream/comm so it overlaps the
        // interior sweep in overlap mode (the host blocks only on these
        // small ops — the interior sweep is already issued)
        allgather_counts(e, (const i64 *)e->d_chg_cnt.get(),
                         /*on_device*/ true, e->h_cntmat, comm, st2);
        // mixed full/compact payload: both ends of every pair decide from
        // the same matrix entry, so the plan is symmetric by construction
        auto full_mode = [](i64 changed, i64 seg) {
            return changed * 12 >= seg * 8;
        };
        // one direction of the plan for peer r: the whole segment, or the
        // (chg_idx, chg_lab) pair of its changed entries, or nothing; the
        // arm taken is counted for mv_halo_info
        struct ArmCounts {
            int64_t &full, &compact, &silent, &entries;
        };
        auto plan = [&](std::vector<Xfer> &out, int r, i64 off, i64 seg,
                        i64 chg, i64 *full, unsigned *idx, i64 *lab,
                        ArmCounts n) {
            if (full_mode(chg, seg)) {
                if (seg > 0) {
                    out.push_back({r, full + off, ncclInt64, seg});
                    n.full++;
                }
            } else if (chg > 0) {
                out.push_back({r, idx + off, ncclChar, chg * 4});
                out.push_back({r, lab + off, ncclInt64, chg});
                n.compact++;
                n.entries += chg;
            } else {
                n.silent++; // seg > 0 here: an empty segment is full_mode
            }
        };
        mv_halo_info &h = e->halo;
        const ArmCounts nsend{h.send_full, h.send_compact, h.send_silent,
                              h.send_compact_entries};
        const ArmCounts nrecv{h.recv_full, h.recv_compact, h.recv_silent,
                              h.recv_compact_entries};
        std::vector<Xfer> sends, recvs;
        for (int r = 0; r < p; r++) {
            if (r == e->rank) continue;
            plan(sends, r, e->send_off[r], e->send_off[r + 1] - e->send_off[r],
                 e->h_cntmat[(i64)e->rank * p + r], e->d_scdata, e->d_chg_idx,
                 e->d_chg_lab, nsend);
            plan(recvs, r, e->recv_off[r], e->recv_off[r + 1] - e->recv_off[r],
                 e->h_cntmat[(i64)r * p + e->rank], e->d_ghost_labels,
                 e->d_rchg_idx, e->d_rchg_lab, nrecv);
        }
        exchange(e, sends, recvs, comm, st2);
        for (int r = 0; r < p; r++) { // scatter compact segments
            if (r == e->rank) continue;
            const i64 rseg = e->recv_off[r + 1] - e->recv_off[r];
            const i64 rchg = e->h_cntmat[(i64)r * p + e->rank];
            if (!full_mode(rchg, rseg) && rchg > 0)
                k_scatter_deltas<<<grid_for(rchg), 256, 0, st2>>>(
                    rchg, e->d_rchg_idx + e->recv_off[r],
                    e->d_rchg_lab + e->recv_off[r], e->recv_off[r],
                    e->d_ghost_labels);
        }
    }
}

// Candidate discovery + halo #1b/#1c/#1d + u32 view build for ONE
// iteration, on (comm, st2): collect the remote communities referenced by
// `curr` / the ghost labels, fetch their (size, degree) records from the
// owners (dspl.hpp:670-929), zero rcu, and build the sweep views. In
// overlap mode this runs on stream2/comm2 during the PREVIOUS iteration's
// epilogue; `ev_cinfo` (when given) gates the reply section on that
// iteration's cinfo updates (K6 + per-sender delta application) — the
// replies must see exactly the reference's post-update localCinfo.
static void halo_prep(mv_engine *e, const i64 *curr,
                      std::vector<i64> &rc_bounds, std::vector<i64> &req_off,
                      i64 &nrc_out, ncclComm_t comm, hipStream_t st2,
                      hipEvent_t ev_cinfo) {
    const int p = e->nranks, me = e->rank;
    const i64 lnv = e->lnv;
    // ---- needed remote communities (dspl.hpp:670-700) ----
    const i64 cand_max = e->nghost + lnv;
    if (e->d_cand.reserve(cand_max)) { // first call after a load
        e->d_cand_sorted.reserve(cand_max);
        e->d_rc_ids.reserve(cand_max);
        e->d_rc_info.reserve(cand_max);
        e->d_rcu.reserve(cand_max);
        size_t t1 = 0, t2 = 0;
        (void)hipcub::DeviceRadixSort::SortKeys(
            nullptr, t1, e->d_cand.get(), e->d_cand_sorted.get(), cand_max, 0,
            e->sort_bits, st2);
        i64 *dummy = nullptr;
        (void)hipcub::DeviceSelect::Unique(nullptr, t2,
                                           e->d_cand_sorted.get(),
                                           e->d_rc_ids.get(), dummy, cand_max,
                                           st2);
        e->d_cub_tmp.reserve((i64)std::max(t1, t2));
    }
    HIP_CHECK(hipMemsetAsync(e->d_count, 0, 8, st2));
    k_filter_remote<<<grid_for(std::max<i64>(e->nghost, 1)), 256, 0, st2>>>(
        e->nghost, e->d_ghost_labels, /*shift*/ 0, e->base, e->bound,
        e->d_cand, e->d_count);
    k_filter_remote<<<grid_for(lnv), 256, 0, st2>>>(
        lnv, curr, /*shift*/ 0, e->base, e->bound, e->d_cand, e->d_count);
    unsigned long long ncand = 0;
    HIP_CHECK(hipMemcpyAsync(&ncand, e->d_count, 8, hipMemcpyDeviceToHost,
                             st2));
    HIP_CHECK(hipStreamSynchronize(st2));
    size_t tb = (size_t)e->d_cub_tmp.cap;
    (void)hipcub::DeviceRadixSort::SortKeys(
        e->d_cub_tmp.get(), tb, e->d_cand.get(), e->d_cand_sorted.get(),
        (int64_t)ncand, 0, e->sort_bits, st2);
    i64 *d_nrc = (i64 *)e->d_count.get(); // reuse as output slot
    tb = (size_t)e->d_cub_tmp.cap;
    (void)hipcub::DeviceSelect::Unique(e->d_cub_tmp.get(), tb,
                                       e->d_cand_sorted.get(),
                                       e->d_rc_ids.get(), d_nrc,
                                       (int64_t)ncand, st2);
    i64 nrc = 0;
    HIP_CHECK(hipMemcpyAsync(&nrc, d_nrc, 8, hipMemcpyDeviceToHost, st2));
    HIP_CHECK(hipStreamSynchronize(st2));

    // ---- halo #1b/#1c/#1d: request (size,degree) of those communities
    // from their owners (dspl.hpp:719-929) ----
    k_owner_bounds<<<1, p + 1, 0, st2>>>(e->d_rc_ids, nrc, e->d_parts, p,
                                         e->d_bounds);
    rc_bounds.assign(p + 1, 0);
    HIP_CHECK(hipMemcpyAsync(rc_bounds.data(), e->d_bounds, 8 * (p + 1),
                             hipMemcpyDeviceToHost, st2));
    HIP_CHECK(hipStreamSynchronize(st2));
    std::vector<i64> reqs(p), matrix((size_t)p * p);
    for (int r = 0; r < p; r++) reqs[r] = rc_bounds[r + 1] - rc_bounds[r];
    allgather_counts(e, reqs.data(), /*on_device*/ false, matrix.data(), comm,
                     st2);
    req_off.assign(p + 1, 0);
    for (int r = 0; r < p; r++)
        req_off[r + 1] =
            req_off[r] + ((r == me) ? 0 : matrix[(size_t)r * p + me]);
    const i64 nreq = req_off[p];
    e->halo.prep_calls++;
    e->halo.nrc_sum += nrc;
    e->halo.nrc_max = std::max<int64_t>(e->halo.nrc_max, nrc);
    if (nrc == 0) e->halo.nrc_zero++;
    e->halo.nreq_sum += nreq;
    if (nreq > e->d_req_ids.cap) { // rare growth; device-wide hipFree sync
                                   // is ok
        e->d_req_ids.reserve(std::max<i64>(nreq, 64));
        e->d_req_info.reserve(std::max<i64>(nreq, 64));
    }
    // the previous iteration's delta routing reads d_req_ids/d_req_info
    // and writes cinfo; #1c's recv and the replies must order after it
    if (ev_cinfo) HIP_CHECK(hipStreamWaitEvent(st2, ev_cinfo, 0));
    alltoallv(e, e->d_rc_ids, rc_bounds.data(), e->d_req_ids, req_off.data(),
              8, ncclInt64, comm, st2);
    k9_reply_info<<<grid_for(std::max<i64>(nreq, 1)), 256, 0, st2>>>(
        nreq, e->d_req_ids, e->base, e->d_sigma_inv, e->d_cinfo,
        e->d_req_info);
    alltoallv(e, e->d_req_info, req_off.data(), e->d_rc_info,
              rc_bounds.data(), sizeof(Info16), ncclChar, comm, st2);
    HIP_CHECK(hipMemsetAsync(e->d_rcu, 0,
                             sizeof(Info16) * std::max<i64>(nrc, 1), st2));
    // u32 views for the sweep (slot / lnv + rc index encoding)
    k_build_view<<<grid_for(lnv), 256, 0, st2>>>(
        lnv, curr, e->base, e->bound, lnv, e->d_sigma_inv, e->d_rc_ids, nrc,
        e->d_vcurr);
    k_build_view<<<grid_for(std::max<i64>(e->nghost, 1)), 256, 0, st2>>>(
        e->nghost, e->d_ghost_labels, e->base, e->bound, lnv,
        e->d_sigma_inv, e->d_rc_ids, nrc, e->d_vghost);
    nrc_out = nrc;
}

// exchangeVertexReqs equivalent (dspl.hpp:1112-1272), the head of the
// timed setup span: ghost discovery, the want-list exchange, the export /
// delta state, the SELL image (p>1) and the global overlap decision.
static void exchange_vertex_reqs(mv_engine *e) {
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv, lne = e->lne;
    const int p = e->nranks, me = e->rank;
    HIP_CHECK(hipMemsetAsync(e->d_count, 0, 8, st));
    if (p == 1) {
        e->nghost = 0;
        e->ssz = 0;
        return; // the SELL image was built at load
    }
    {
        DevBuf<i64> d_rem, d_sorted, d_ng; // temporaries: freed with this
        DevBuf<char> d_tmp;                // block
        d_rem.reserve(lne);
        k_select_remote<<<grid_for(lne), 256, 0, st>>>(
            lne, e->d_tails, e->base, e->bound, d_rem, e->d_count);
        unsigned long long nrem = 0;
        HIP_CHECK(hipMemcpyAsync(&nrem, e->d_count, 8, hipMemcpyDeviceToHost,
                                 st));
        HIP_CHECK(hipStreamSynchronize(st));
        // sort + unique -> ghosts
        d_sorted.reserve((i64)nrem);
        e->d_ghosts.reserve((i64)nrem);
        d_ng.reserve(1);
        size_t tmp1 = 0, tmp2 = 0;
        (void)hipcub::DeviceRadixSort::SortKeys(
            nullptr, tmp1, d_rem.get(), d_sorted.get(), (int64_t)nrem, 0,
            e->sort_bits, st);
        (void)hipcub::DeviceSelect::Unique(nullptr, tmp2, d_sorted.get(),
                                           e->d_ghosts.get(), d_ng.get(),
                                           (int64_t)nrem, st);
        d_tmp.reserve((i64)std::max(tmp1, tmp2));
        (void)hipcub::DeviceRadixSort::SortKeys(
            d_tmp.get(), tmp1, d_rem.get(), d_sorted.get(), (int64_t)nrem, 0,
            e->sort_bits, st);
        (void)hipcub::DeviceSelect::Unique(d_tmp.get(), tmp2, d_sorted.get(),
                                           e->d_ghosts.get(), d_ng.get(),
                                           (int64_t)nrem, st);
        HIP_CHECK(hipMemcpyAsync(&e->nghost, d_ng, 8, hipMemcpyDeviceToHost,
                                 st));
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // per-owner segments of my (sorted) want list
    k_owner_bounds<<<1, p + 1, 0, st>>>(e->d_ghosts, e->nghost, e->d_parts, p,
                                        e->d_bounds);
    e->recv_off.resize(p + 1);
    HIP_CHECK(hipMemcpyAsync(e->recv_off.data(), e->d_bounds, 8 * (p + 1),
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));

    // exchange want-list sizes, then the lists (dspl.hpp:1184-1252)
    std::vector<i64> want(p), matrix((size_t)p * p);
    for (int r = 0; r < p; r++) want[r] = e->recv_off[r + 1] - e->recv_off[r];
    allgather_counts(e, want.data(), /*on_device*/ false, matrix.data(),
                     e->comm, st);
    e->send_off.assign(p + 1, 0);
    for (int r = 0; r < p; r++)
        e->send_off[r + 1] =
            e->send_off[r] + ((r == me) ? 0 : matrix[(size_t)r * p + me]);
    e->ssz = e->send_off[p];
    e->d_svdata.reserve(e->ssz);
    e->d_svdata_int.reserve(e->ssz);
    // role swap (dspl.hpp:1255-1257): my ghost list goes OUT, the peers'
    // lists land in svdata
    alltoallv(e, e->d_ghosts, e->recv_off.data(), e->d_svdata,
              e->send_off.data(), 8, ncclInt64, e->comm, st);
    k_to_internal<<<grid_for(std::max<i64>(e->ssz, 1)), 256, 0, st>>>(
        e->ssz, e->d_svdata, e->base, e->d_sigma_inv, e->d_svdata_int);
    HIP_CHECK(hipStreamSynchronize(st));

    e->d_vghost.reserve(e->nghost);
    e->d_vcurr.reserve(lnv);
    e->d_vtarget.reserve(lnv);
    e->d_scdata.reserve(e->ssz);

    // delta-compaction state (default on; MV_NO_DELTA reverts to the
    // reference's full resend for A/B). The buffers are reused across
    // runs; every run starts from "all changed" (d_last_sent = -1), so
    // iteration 1 resends every segment in full and nothing reads what a
    // previous run left in the others.
    e->use_delta = !getenv("MV_NO_DELTA");
    e->d_last_sent.reserve(e->ssz);
    HIP_CHECK(hipMemsetAsync(e->d_last_sent, 0xFF,
                             8 * std::max<i64>(e->ssz, 1), st));
    e->d_chg_idx.reserve(e->ssz);
    e->d_chg_lab.reserve(e->ssz);
    e->d_chg_cnt.reserve(p);
    e->d_soff.reserve(p + 1);
    HIP_CHECK(hipMemcpyAsync(e->d_soff, e->send_off.data(), 8 * (p + 1),
                             hipMemcpyHostToDevice, st));
    e->d_ghost_labels.reserve(e->nghost);
    e->d_rchg_idx.reserve(e->nghost);
    e->d_rchg_lab.reserve(e->nghost);
    e->h_cntmat.reserve((i64)p * p);
    HIP_CHECK(hipStreamSynchronize(st));

    build_sell(e);
    // overlap changes the collective sequence, so it must be a GLOBAL
    // decision: all ranks take it or none (a rank can be locally skewed /
    // export-free while others are not)
    std::vector<i64> flag(p, e->overlap ? 1 : 0);
    allgather_counts(e, flag.data(), /*on_device*/ false, matrix.data(),
                     e->comm, st);
    for (int r = 0; r < p; r++)
        if (matrix[(size_t)r * p] == 0) e->overlap = 0;
}

#define PHASE(tag)                                                            \
    do {                                                                      \
        if (getenv("MV_PHASE_DEBUG")) {                                       \
            HIP_CHECK(hipStreamSynchronize(e->stream));                       \
            std::fprintf(stderr, "[phase] %s\n", tag);                        \
            std::fflush(stderr);                                              \
        }                                                                     \
    } while (0)

double mv_engine_run(mv_engine *e, double lower, double thresh,
                     int *iters_out) {
    HIP_CHECK(hipSetDevice(e->device));
    const auto t_start = std::chrono::steady_clock::now();
    hipStream_t st = e->stream;
    const i64 lnv = e->lnv, lne = e->lne;
    const int p = e->nranks;
    e->ev_used = 0;
    e->stats = mv_stats{};
    e->sweep = mv_sweep_info{};
    e->halo = mv_halo_info{};
    e->stats.edges_local = lne;

    const auto t_setup0 = std::chrono::steady_clock::now();
    exchange_vertex_reqs(e);

    PHASE("setup-done");
    // ---- distInitLouvain (dspl.hpp:151-172) ----
    k1_vertex_degree<<<grid_for(lnv), 256, 0, st>>>(
        lnv, e->d_sigma, e->d_xadj, e->d_ew, e->unit_weights, e->d_vdeg,
        e->d_cinfo);
    PHASE("k1-done");
    const int nblocks = grid_for(lnv);
    {
        auto f = [vd = e->d_vdeg.get()] __device__(i64 i, double &a,
                                                   double &b) {
            a = vd[i];
            b = 0.0;
        };
        k_partial_sum2<<<nblocks, 256, 0, st>>>(lnv, f, e->d_partials);
    }
    double *const partials = e->h_partials;
    HIP_CHECK(hipMemcpyAsync(partials, e->d_partials, 16 * nblocks,
                             hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    double localW = 0.0;
    for (int b = 0; b < nblocks; b++) localW += partials[2 * b];
    double totalW = localW;
    if (p > 1) comm_allreduce_host(e, &totalW, 1); // allreduce (dspl.hpp:126)
    const double constant = 1.0 / totalW; // dspl.hpp:129
    PHASE("k2-done");
    if (p == 1) // slot mode: the i64 arrays alias u32 slot arrays
        k3_init_comm32<<<grid_for(lnv), 256, 0, st>>>(
            lnv, (unsigned *)e->d_curr.get(), (unsigned *)e->d_past.get());
    else
        k3_init_comm<<<grid_for(lnv), 256, 0, st>>>(lnv, e->base, e->d_sigma,
                                                    e->d_curr, e->d_past);
    HIP_CHECK(hipStreamSynchronize(st));
    PHASE("k3-done");
    e->stats.setup_ms =
        std::chrono::duration<double, std::milli>(
            std::chrono::steady_clock::now() - t_setup0)
            .count();

    i64 *d_curr = e->d_curr, *d_past = e->d_past, *d_target = e->d_target;
    double prevMod = lower, currMod = -1.0;
    int numIters = 0;
    // halo state for the CURRENT iteration, and the one the overlapped
    // pipeline prepares for the NEXT (swapped at each loop top)
    std::vector<i64> rc_bounds(p + 1, 0), req_off(p + 1, 0);
    std::vector<i64> rc_bounds_nx(p + 1, 0), req_off_nx(p + 1, 0);
    i64 nrc = 0, nrc_nx = 0;

    // Overlap mode: the ENTIRE next-iteration halo pipeline — #1a ghost
    // communities off the exports' targets, candidate discovery, counts,
    // #1c/#1d info fetch, rcu zero and the view builds — runs on
    // stream2/comm2 while stream A sweeps the interior and runs the
    // epilogue; only #2 + the modularity allreduce stay on the critical
    // path. Joined via ev_halo at the next iteration's top.
    ncclComm_t c2 = e->comm2 ? e->comm2 : e->comm;
    if (p > 1 && e->overlap) {
        HIP_CHECK(hipEventRecord(e->ev_p1, st));
        HIP_CHECK(hipStreamWaitEvent(e->stream2, e->ev_p1, 0));
        run_halo1a(e, e->d_curr, c2, e->stream2);
        halo_prep(e, e->d_curr, rc_bounds, req_off, nrc, c2, e->stream2,
                  nullptr); // initial cinfo (K1) is complete: A was synced
        HIP_CHECK(hipEventRecord(e->ev_halo, e->stream2));
    }

    std::vector<hipEvent_t> sweep_ev;
    for (;;) {
        numIters++;

        if (p > 1) {
            const auto t_h0 = std::chrono::steady_clock::now();
            if (e->overlap) {
                // pipeline prepared everything during the previous
                // iteration's epilogue (or pre-loop)
                HIP_CHECK(hipStreamWaitEvent(st, e->ev_halo, 0));
                if (numIters > 1) {
                    std::swap(rc_bounds, rc_bounds_nx);
                    std::swap(req_off, req_off_nx);
                    nrc = nrc_nx;
                }
            } else {
                run_halo1a(e, d_curr, e->comm, st);
                halo_prep(e, d_curr, rc_bounds, req_off, nrc, e->comm, st,
                          nullptr);
                HIP_CHECK(hipStreamSynchronize(st));
            }
            e->stats.halo_ms +=
                std::chrono::duration<double, std::milli>(
                    std::chrono::steady_clock::now() - t_h0)
                    .count();
        }

        // ---- K4 sweep (dspl.hpp:1371-1387; K5's zeroing is fused: cupd is
        // zeroed by K6 after each apply + once before the loop, and the
        // sweep overwrites clusterWeight instead of accumulating) ----
        if (numIters == 1 && lnv)
            HIP_CHECK(hipMemsetAsync(e->d_cupd, 0, sizeof(Cinfo) * lnv, st));
        hipEvent_t ev0 = e->ev_pair(), ev1 = e->ev_pair();
        HIP_CHECK(hipEventRecord(ev0, st));
        // LDS slots per lane: early iterations see ~degree distinct
        // candidate communities (every vertex its own community), later
        // ones only a handful — a larger-slot / lower-occupancy variant for
        // the first iterations avoids the spill path where it matters.
        // Tunables (perf only, results identical): MV_SLOTS, MV_SLOTS_FIRST,
        // MV_FIRST_ITERS.
        static const int slots_env = [] {
            const char *s = getenv("MV_SLOTS");
            return s ? atoi(s) : 0;
        }();
        static const int slots_first_env = [] {
            const char *s = getenv("MV_SLOTS_FIRST");
            return s ? atoi(s) : -1;
        }();
        // Degree-adaptive defaults: RGG-class graphs (deg ~10) measured
        // best at 8 slots (12 first iterations at p==1); dense social
        // shapes (deg ~70, ~25 persistent distinct candidates from long-
        // range edges) at 24 (72 KiB/block, 2 blocks/CU) — +23% on the
        // orkut_like workload, while 32+ falls off the occupancy cliff
        // (experiments/RESULTS.md).
        const bool dense = lne > 16 * lnv;
        const int slots_rest = slots_env > 0 ? slots_env : (dense ? 24 : 8);
        const int slots_first =
            slots_first_env > 0
                ? slots_first_env
                : (dense ? 24 : ((p == 1) ? 12 : slots_rest));
        static const int first_iters = [] {
            const char *s = getenv("MV_FIRST_ITERS");
            return s ? atoi(s) : 2;
        }();
        const int slots = (numIters <= first_iters) ? slots_first : slots_rest;
        // Mode (the kernels' MR): view mode at p>1; at p==1 slot mode,
        // where the u32 slot arrays ARE the view and the ghost/rc
        // pointers are load_graph's never-read dummies (d_ghosts: null).
        // by_flag turns a run-time bool into a std::bool_constant tag.
        auto by_flag = [](bool b, auto f) {
            if (b) f(std::true_type{});
            else f(std::false_type{});
        };
        const unsigned *vcurr = p == 1 ? (const unsigned *)d_curr : e->d_vcurr;
        unsigned *vtarget = p == 1 ? (unsigned *)d_target : e->d_vtarget;
        auto range_grid = [&](i64 s0, i64 s1) {
            return p == 1 ? e->sweep_grid
                          : grid_for(s1 - s0, 256, e->sweep_grid);
        };
        // Row schedule of a lane-per-vertex launch. By default the queue
        // serves the general sweep from iteration first_iters + 1 on: in
        // the first iterations nearly every vertex moves, the tickets then
        // wait behind the moves' own cupd atomics and the queue loses
        // (measured, experiments/RESULTS.md). MV_SWEEP_QUEUE_FROM moves
        // that first iteration (tests reach the queue on graphs that
        // converge in two). k4_sweep_iter1 and the launches that do not
        // queue keep the static schedule and the full grid.
        const RowQueue static_rows{nullptr, {}, e->row_group, 0};
        const bool queued =
            e->sched_unit > 0 &&
            numIters >= (e->sched_from ? e->sched_from : first_iters + 1);
        // the queue's launch view; the host totals advance by the tickets
        // the launch will consume, nu in all (see RowQueue)
        auto take_queue = [&](i64 s0, i64 s1, int grid) {
            RowQueue q{e->d_ticket, {}, e->sched_unit, 1};
            while (q.heads * 2 <= std::min(grid, QUEUE_HEADS)) q.heads *= 2;
            const i64 H = q.heads;
            const i64 rows = (s1 - s0 + 63) / 64;
            const i64 nu = (rows + q.unit - 1) / q.unit, nw = 4 * (i64)grid;
            const i64 nq = std::max<i64>(nu - nw, 0); // queued units
            const i64 m = std::min(nu, nw); // waves with a first unit: each
                                            // ends on one dry ticket
            auto share = [H](i64 n, i64 h) { // |{j < n : j % H == h}|
                return n > h ? (n - h + H - 1) / H : 0;
            };
            for (i64 h = 0; h < H; h++) {
                q.base[h] = (unsigned)e->tickets_total[h];
                e->tickets_total[h] += share(nq, h) + 4 * share(m / 4, h) +
                                       ((m / 4) % H == h ? m % 4 : 0);
            }
            return q;
        };
        auto launch_sweep = [&](auto mr_tag, auto slots_tag, auto unit_tag,
                                auto idp_tag, i64 s0, i64 s1) {
            constexpr int S = decltype(slots_tag)::value; // 12 B/lane LDS
            const auto kernel = k4_sweep<decltype(mr_tag)::value, S,
                                         decltype(unit_tag)::value,
                                         decltype(idp_tag)::value>;
            e->sweep.general++;
            e->sweep.general_slots[mv_sweep_slot_index(S)]++;
            int grid = range_grid(s0, s1);
            if (queued) {
                // one resident round: a first unit on a block that starts
                // late is a unit no other wave can take
                int &per_cu = e->sweep_per_cu[mv_sweep_slot_index(S)]
                                             [decltype(unit_tag)::value]
                                             [decltype(idp_tag)::value];
                if (!per_cu) { // once per engine and instantiation
                    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
                        &per_cu, kernel, 256, S * 256 * 12));
                    per_cu = std::max(per_cu, 1);
                }
                grid = std::min(grid, per_cu * e->num_cus);
            }
            if (s1 == lnv) e->sched_grid = grid;
            kernel<<<grid, 256, S * 256 * 12, st>>>(
                s0, s1, lnv, e->base, e->d_perm, e->d_deg, e->d_chunk_off,
                e->d_sell_tidx, e->d_sell_w, vcurr, e->d_vghost, e->d_vdeg,
                e->d_sigma, e->d_cinfo, e->d_cupd, e->d_rc_ids, e->d_rc_info,
                e->d_rcu, constant, vtarget, e->d_cw,
                (unsigned *)e->d_spill_k.get(), e->d_spill_a, e->d_spill_off,
                queued ? take_queue(s0, s1, grid) : static_rows);
        };
        auto dispatch_slots = [&](auto mr_tag, auto unit_tag, i64 s0,
                                  i64 s1) {
            auto go = [&](auto slots_tag) {
                by_flag(e->perm_identity, [&](auto idp_tag) {
                    launch_sweep(mr_tag, slots_tag, unit_tag, idp_tag, s0,
                                 s1);
                });
            };
            switch (slots) {
            case 4: go(std::integral_constant<int, 4>{}); break;
            case 12: go(std::integral_constant<int, 12>{}); break;
            case 16: go(std::integral_constant<int, 16>{}); break;
            case 24: go(std::integral_constant<int, 24>{}); break;
            case 32: go(std::integral_constant<int, 32>{}); break;
            case 48: go(std::integral_constant<int, 48>{}); break;
            default: go(std::integral_constant<int, 8>{}); break;
            }
        };
        auto launch_iter1 = [&](auto mr_tag, auto unit_tag, auto lblasc_tag,
                                i64 s0, i64 s1) {
            if (decltype(lblasc_tag)::value) e->sweep.iter1_label_order++;
            else e->sweep.iter1_internal_order++;
            by_flag(e->perm_identity, [&](auto idp_tag) {
                k4_sweep_iter1<decltype(mr_tag)::value,
                               decltype(unit_tag)::value,
                               decltype(lblasc_tag)::value,
                               decltype(idp_tag)::value>
                    <<<range_grid(s0, s1), 256, 0, st>>>(
                        s0, s1, lnv, e->base, e->d_perm, e->d_deg,
                        e->d_chunk_off, e->d_sell_tidx, e->d_sell_w,
                        e->d_vghost, e->d_ghosts, e->d_vdeg, e->d_sigma,
                        e->d_cupd, e->d_rc_info, e->d_rcu, constant, vtarget,
                        e->d_cw, e->row_group);
            });
        };
        if (e->nlh > 0) { // hash-aggregation bands (skewed graphs)
            HIP_CHECK(hipMemsetAsync(e->d_hkeys, 0xFF, 8 * e->hash_total,
                                     st));
            if (e->hash_hub_elems) // the wave kernel atomic-adds into its
                                   // prefix; the lane band writes on insert
                HIP_CHECK(hipMemsetAsync(e->d_hacc, 0,
                                         8 * e->hash_hub_elems, st));
            if (e->nlh > e->nhi) // per-lane hash band [nhi, nlh)
                by_flag(e->unit_weights, [&](auto unit_tag) {
                    e->sweep.lh++;
                    k4_sweep_lh<decltype(unit_tag)::value>
                        <<<grid_for(e->nlh - e->nhi), 256, 0, st>>>(
                            e->nhi, e->nlh, lnv, e->base, e->d_perm,
                            e->d_deg, e->d_chunk_off, e->d_sell_tidx,
                            e->d_sell_w, vcurr, e->d_vghost, e->d_vdeg,
                            e->d_sigma, e->d_cinfo, e->d_cupd, e->d_rc_ids,
                            e->d_rc_info, e->d_rcu, constant, vtarget,
                            e->d_cw, e->d_hash_off, e->d_hkeys, e->d_hacc,
                            e->d_lh_list);
                });
            if (e->nhi > 0) // wave-per-vertex hubs [0, nhi)
                by_flag(p > 1, [&](auto mr_tag) {
                    e->sweep.hi++;
                    k4_sweep_hi<decltype(mr_tag)::value>
                        <<<grid_for(e->nhi * 64, 256, 2048), 256, 0, st>>>(
                            e->nhi, lnv, e->base, e->d_perm, e->d_deg,
                            e->d_sigma, e->d_xadj, e->d_tidx32, vcurr,
                            e->d_vghost, e->d_vdeg, e->d_cinfo, e->d_cupd,
                            e->d_rc_ids, e->d_rc_info, e->d_rcu, constant,
                            vtarget, e->d_cw, e->d_hash_off, e->d_hkeys,
                            e->d_hacc);
                });
        }
        static const bool no_iter1 = getenv("MV_NO_ITER1") != nullptr;
        auto sweep_range = [&](i64 s0, i64 s1) {
            if (s1 <= s0) return;
            const std::true_type yes{};
            const std::false_type no{};
            by_flag(p > 1, [&](auto mr_tag) {
                if (numIters == 1 && (e->rows_sorted || e->sell_sorted) &&
                    !no_iter1) {
                    if (e->sell_sorted) // internal order: explicit label ties
                        launch_iter1(mr_tag, yes, no, s0, s1);
                    else if (e->unit_weights)
                        launch_iter1(mr_tag, yes, yes, s0, s1);
                    else
                        launch_iter1(mr_tag, no, yes, s0, s1);
                } else {
                    by_flag(e->unit_weights, [&](auto unit_tag) {
                        dispatch_slots(mr_tag, unit_tag, s0, s1);
                    });
                }
            });
        };
        // persist the sweep's u32 view targets as labels (p>1 only)
        auto writeback = [&](i64 s0, i64 s1) {
            if (p == 1 || s1 <= s0) return;
            k_view_to_labels<<<grid_for(s1 - s0, 256, 2048), 256, 0, st>>>(
                s0, s1, e->d_perm, e->d_vtarget, e->d_sigma, e->base,
                e->d_rc_ids, lnv, d_target);
        };
        if (p > 1 && e->overlap) {
            // exports first (their targets feed the next iteration's #1a
            // once ev_p1 fires); the full next-iteration pipeline is
            // issued after the epilogue's delta application (ev_cinfo) so
            // it runs under the epilogue + exit check — see below
            sweep_range(0, e->nexp);
            writeback(0, e->nexp);
            HIP_CHECK(hipEventRecord(e->ev_p1, st));
            sweep_range(e->nexp, lnv);
            writeback(e->nexp, lnv);
            HIP_CHECK(hipEventRecord(e->ev_p2, st));
        } else {
            sweep_range(e->nlh, lnv);
            writeback(0, lnv);
        }
        HIP_CHECK(hipEventRecord(ev1, st));
        PHASE("sweep-done");
        sweep_ev.push_back(ev0);
        sweep_ev.push_back(ev1);
        e->stats.sweep_launches++;

        // (phase markers around K6/K7 below)
        // ---- K6 (dspl.hpp:458-471); fused with K7 at p==1 ----
        if (p == 1) {
            k67_apply_and_partials<<<nblocks, 256, 0, st>>>(
                lnv, e->d_cupd, e->d_cinfo, e->d_cw, e->d_partials);
        } else {
            k6_apply_local<<<grid_for(lnv), 256, 0, st>>>(lnv, e->d_cupd,
                                                          e->d_cinfo);
        }

        // ---- halo #2: route deltas to owners (dspl.hpp:978-1103) ----
        if (p > 1) {
            const auto t_h0 = std::chrono::steady_clock::now();
            alltoallv(e, e->d_rcu, rc_bounds.data(), e->d_req_info,
                      req_off.data(), sizeof(Info16), ncclChar, e->comm,
                      e->stream);
            // apply per SENDER segment, in rank order: same-stream launches
            // serialize, and one sender's ids are unique (sorted rc_ids), so
            // cinfo degree bits are run-to-run identical at any nranks —
            // like the reference's in-order delta walk (dspl.hpp:1089-1102)
            for (int r = 0; r < p; r++) {
                const i64 c = req_off[r + 1] - req_off[r];
                if (c > 0)
                    k_apply_deltas<<<grid_for(c), 256, 0, st>>>(
                        c, e->d_req_ids + req_off[r], e->base, e->d_sigma_inv,
                        e->d_req_info + req_off[r], e->d_cinfo);
            }
            if (e->overlap) {
                // the next-iteration pipeline's replies must see THIS
                // post-update cinfo and may reuse the req buffers after it
                HIP_CHECK(hipEventRecord(e->ev_cinfo, st));
            } else {
                HIP_CHECK(hipStreamSynchronize(st));
            }
            e->stats.halo_ms +=
                std::chrono::duration<double, std::milli>(
                    std::chrono::steady_clock::now() - t_h0)
                    .count();
        }

        // ---- K7: modularity (dspl.hpp:407-456; p==1 already emitted the
        // partials in the fused kernel above) ----
        if (p > 1) {
            auto f = [cw = e->d_cw.get(), ci = e->d_cinfo.get()] __device__(
                         i64 i, double &a, double &b) {
                a = cw[i];
                const double d = ci[i].degree;
                b = d * d;
            };
            k_partial_sum2<<<nblocks, 256, 0, st>>>(lnv, f, e->d_partials);
        }
        PHASE("k67-done");
        HIP_CHECK(hipMemcpyAsync(partials, e->d_partials, 16 * nblocks,
                                 hipMemcpyDeviceToHost, st));
        if (p > 1 && e->overlap) {
            // issue the WHOLE next-iteration halo pipeline on stream2 now
            // (A's epilogue is queued and drains concurrently): #1a off
            // the exports (ev_p1), discovery off the full targets (ev_p2),
            // replies off the updated cinfo (ev_cinfo)
            HIP_CHECK(hipStreamWaitEvent(e->stream2, e->ev_p1, 0));
            run_halo1a(e, d_target, c2, e->stream2);
            HIP_CHECK(hipStreamWaitEvent(e->stream2, e->ev_p2, 0));
            halo_prep(e, d_target, rc_bounds_nx, req_off_nx, nrc_nx, c2,
                      e->stream2, e->ev_cinfo);
            HIP_CHECK(hipEventRecord(e->ev_halo, e->stream2));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        double le = 0.0, la = 0.0;
        for (int b = 0; b < nblocks; b++) {
            le += partials[2 * b];
            la += partials[2 * b + 1];
        }
        double red[2] = {le, la};
        if (p > 1) comm_allreduce_host(e, red, 2);
        currMod = std::fabs(red[0] * constant - red[1] * constant * constant);
        if (getenv("MV_MOD_DEBUG"))
            std::fprintf(stderr, "[mod] iter=%d le=%.17g la=%.17g\n",
                         numIters, red[0], red[1]);

        // ---- trace ----
        if (e->trace_mod && numIters <= e->trace_cap)
            e->trace_mod[numIters - 1] = currMod;
        if (e->trace_target && numIters <= e->trace_cap) {
            if (p == 1)
                k_depermute32<<<grid_for(lnv), 256, 0, st>>>(
                    lnv, e->d_sigma, e->d_sigma_inv,
                    (const unsigned *)d_target, e->d_trace_tmp);
            else
                k_depermute<<<grid_for(lnv), 256, 0, st>>>(
                    lnv, e->d_sigma_inv, d_target, e->d_trace_tmp);
            if (lnv)
                HIP_CHECK(hipMemcpyAsync(e->trace_target +
                                             (i64)(numIters - 1) * lnv,
                                         e->d_trace_tmp, 8 * lnv,
                                         hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }

        if (currMod - prevMod < thresh) break; // dspl.hpp:1401
        prevMod = currMod;
        if (prevMod < lower) prevMod = lower; // dspl.hpp:1404-1406
        // rotate (dspl.hpp:1417-1422): every array is fully rewritten or
        // never read, so pointer rotation is equivalent to the content swap
        i64 *tmp = d_past;
        d_past = d_curr;
        d_curr = d_target;
        d_target = tmp;
        if (numIters >= 10000) break; // safety net, never hit in practice
    }
    // overlap mode posted one speculative #1a past the exit; every rank
    // posted it symmetrically — drain it before returning
    if (e->overlap) HIP_CHECK(hipStreamSynchronize(e->stream2));

    const bool dbg = getenv("MV_SWEEP_DEBUG") != nullptr;
    for (size_t k = 0; k + 1 < sweep_ev.size() + 1; k += 2) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, sweep_ev[k], sweep_ev[k + 1]));
        e->stats.sweep_ms += ms;
        if (dbg)
            std::fprintf(stderr, "[sweep] iter %zu: %.3f ms\n", k / 2 + 1, ms);
    }
    e->res_src = numIters <= 2 ? d_curr : d_past;
    e->stats.iters = numIters;
    e->stats.total_ms = std::chrono::duration<double, std::milli>(
                            std::chrono::steady_clock::now() - t_start)
                            .count();
    *iters_out = numIters;
    return prevMod; // dspl.hpp:1440
}

} // extern "C"

// ------------------------------------------------------------------------
// Phase assignment + multi-phase driver (multi-phase section).
// The reference mini-app stops after phase one; nothing below has a
// counterpart there.

// The last run's phase assignment as LABELS in original local order, in
// e->d_res (device). Null before the first run.
static const i64 *phase_labels_device(mv_engine *e) {
    if (!e->res_src) return nullptr;
    const i64 lnv = e->lnv;
    e->d_res.reserve(lnv);
    if (e->nranks == 1)
        k_depermute32<<<grid_for(lnv), 256, 0, e->stream>>>(
            lnv, e->d_sigma, e->d_sigma_inv, (const unsigned *)e->res_src,
            e->d_res);
    else
        k_depermute<<<grid_for(lnv), 256, 0, e->stream>>>(
            lnv, e->d_sigma_inv, e->res_src, e->d_res);
    return e->d_res;
}

// q of a level's graph: sum_c selfloop_c / W - sum_c deg_c^2 / W^2, in
// row order on the host (levels are host-resident anyway)
static double level_modularity(const mv_graph *g) {
    const i64 nv = mv_graph_lnv(g);
    const i64 *xadj = mv_graph_xadj(g), *tails = mv_graph_tails(g);
    const double *w = mv_graph_weights(g);
    double W = 0.0, loops = 0.0, deg2 = 0.0;
    for (i64 v = 0; v < nv; v++) {
        double d = 0.0;
        for (i64 k = xadj[v]; k < xadj[v + 1]; k++) {
            d += w[k];
            if (tails[k] == v) loops += w[k];
        }
        W += d;
        deg2 += d * d;
    }
    return W == 0.0 ? 0.0 : loops / W - deg2 / (W * W);
}

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

static int id_bits(i64 nv) {
    int b = 1;
    while ((1ll << b) < nv) b++;
    return b;
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
    std::vector<i64> soff(p + 1), roff(p + 1, 0), cnt(p),
        m((size_t)p * p);
    mv_lower_bounds(st, (const uint64_t *)d_uniq, nuniq, keys.data(), p + 1,
                    soff.data());
    for (int r = 0; r < p; r++) cnt[r] = soff[r + 1] - soff[r];
    gather_counts(e, cnt.data(), m.data());
    for (int r = 0; r < p; r++)
        roff[r + 1] = roff[r] + (r == me ? 0 : m[(size_t)r * p + me]);
    const i64 nreq = roff[p];
    DevBuf<i64> d_req, d_rep;
    d_req.reserve(nreq);
    d_rep.reserve(nreq);
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
    mv_sort_unique_ids(e->stream, n, d_ids, id_bits(nv), &u);
    DevBuf<i64> d_vals;
    d_vals.reserve(u.nuniq);
    dist_fetch(e, parts, u.d_uniq, u.nuniq, d_table, d_vals);
    mv_scatter_unique(e->stream, &u, d_vals, d_out);
    HIP_CHECK(hipStreamSynchronize(e->stream));
    mv_unique_ids_free(&u);
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
    const int bits = id_bits(nv);
    std::vector<i64> soff(p + 1, 0), roff(p + 1, 0), cnt(p),
        m((size_t)p * p);
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
        DevBuf<i64> d_lab;
        DevBuf<unsigned> d_err;
        d_lab.reserve(lnv);
        d_err.reserve(1);
        HIP_CHECK(hipMemsetAsync(d_err, 0, 4, st));
        mv_check_labels(st, lnv, d_labels, nv, d_lab, d_err);
        unsigned h_err = 0;
        HIP_CHECK(hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (h_err) {
            std::fprintf(stderr,
                         "coarsen (rank %d): community label outside "
                         "[0, nv=%lld)\n",
                         me, (long long)nv);
            bad = true;
        } else {
            mv_sort_unique_ids(st, lnv, d_lab, bits, &u);
            for (int r = 0; r <= p; r++) keys[r] = (uint64_t)parts[r];
            mv_lower_bounds(st, (const uint64_t *)u.d_uniq, u.nuniq,
                            keys.data(), p + 1, soff.data());
        }
    }
    for (int r = 0; r < p; r++) cnt[r] = bad ? -1 : soff[r + 1] - soff[r];
    gather_counts(e, cnt.data(), m.data());
    for (size_t k = 0; k < m.size(); k++)
        if (m[k] < 0) { // some rank refused: everyone does, before any send
            mv_unique_ids_free(&u);
            return -1;
        }
    for (int r = 0; r < p; r++)
        roff[r + 1] = roff[r] + (r == me ? 0 : m[(size_t)r * p + me]);
    i64 nc = 0, offset = 0;
    DevBuf<i64> d_dense; // dense coarse id of every owned label in use
    {
        const i64 nreq = roff[p];
        DevBuf<i64> d_req;
        DevBuf<unsigned> d_used, d_rank;
        d_req.reserve(nreq);
        d_used.reserve(lnv + 1);
        d_rank.reserve(lnv + 1);
        a2a64(e, u.d_uniq, soff.data(), d_req, roff.data());
        HIP_CHECK(hipMemsetAsync(d_used, 0, 4 * (lnv + 1), st));
        mv_mark_owned(st, nreq, d_req, base, d_used);
        mv_mark_owned(st, cnt[me], u.d_uniq + soff[me], base, d_used);
        mv_exclusive_sum_u32(st, d_used, d_rank, lnv + 1);
        unsigned h_cnt = 0;
        HIP_CHECK(hipMemcpyAsync(&h_cnt, d_rank + lnv, 4,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<i64> mine(p, (i64)h_cnt);
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
        DevBuf<i64> d_vals;
        d_vals.reserve(u.nuniq);
        dist_fetch(e, parts, u.d_uniq, u.nuniq, d_dense, d_vals);
        mv_scatter_unique(st, &u, d_vals, out->d_map);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    mv_unique_ids_free(&u);
    out->nc = nc;
    out->parts.resize(p + 1);
    for (int r = 0; r <= p; r++) out->parts[r] = (nc * r) / p;
    out->lnc = out->parts[me + 1] - out->parts[me];
    if (stop_if_identity && nc == nv) return 0;

    // ---- (b) coarse ids of the tails: remote ones are fetched ----
    mv_unique_ids gh;
    DevBuf<i64> d_gmap;
    {
        DevBuf<i64> d_rem;
        DevBuf<unsigned long long> d_nrem;
        d_rem.reserve(lne);
        d_nrem.reserve(1);
        HIP_CHECK(hipMemsetAsync(d_nrem, 0, 8, st));
        k_select_remote<<<grid_for(lne), 256, 0, st>>>(lne, d_tails, base,
                                                       bound, d_rem, d_nrem);
        unsigned long long nrem = 0;
        HIP_CHECK(hipMemcpyAsync(&nrem, d_nrem, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        mv_sort_unique_ids(st, (i64)nrem, d_rem, bits, &gh);
    }
    d_gmap.reserve(gh.nuniq);
    dist_fetch(e, parts, gh.d_uniq, gh.nuniq, out->d_map, d_gmap);

    // ---- keys, local sort + run reduction: one partial per local pair ----
    int shift = 1;
    while ((1ll << shift) < nc) shift++;
    mv_key_runs part;
    {
        DevBuf<uint64_t> d_keys;
        d_keys.reserve(lne);
        mv_coarse_keys_dist(st, lnv, lne, d_xadj, d_tails, base, bound,
                            out->d_map, gh.d_uniq, gh.nuniq, d_gmap, shift,
                            d_keys);
        mv_sort_reduce_keys(st, lne, d_keys, d_w, 2 * shift, &part);
    }
    mv_unique_ids_free(&gh);

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
            mv_key_runs_free(&part);
            return -1;
        }
    }
    // segments by ascending sender, my own in its place: the stable sort
    // then adds the per-rank partials of a pair in rank order
    for (int r = 0; r < p; r++) roff[r + 1] = roff[r] + m[(size_t)r * p + me];
    const i64 nrecv = roff[p];
    mv_key_runs fin;
    {
        DevBuf<uint64_t> d_rk;
        DevBuf<double> d_rw;
        d_rk.reserve(nrecv);
        d_rw.reserve(nrecv);
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
    mv_key_runs_free(&part);
    out->ne = fin.n;
    out->d_xadj.reserve(out->lnc + 1);
    out->d_tails.reserve(fin.n);
    mv_coarse_rows(st, out->parts[me], out->lnc, fin.n, shift, fin.d_key,
                   out->d_xadj, out->d_tails);
    HIP_CHECK(hipStreamSynchronize(st));
    // the run weights ARE the coarse weights (never fewer than 1 element)
    out->d_w.adopt(fin.d_w, std::max<i64>(fin.n, 1));
    fin.d_w = nullptr;
    mv_key_runs_free(&fin);
    return 0;
}

// the coarse slice as a host level (parts = the even split)
static mv_graph *level_from_device(mv_engine *e, const DistCoarse &c) {
    std::vector<i64> cx(c.lnc + 1), ct(c.ne);
    std::vector<double> cw(c.ne);
    HIP_CHECK(hipMemcpy(cx.data(), c.d_xadj, 8 * (c.lnc + 1),
                        hipMemcpyDeviceToHost));
    if (c.ne) {
        HIP_CHECK(hipMemcpy(ct.data(), c.d_tails, 8 * c.ne,
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cw.data(), c.d_w, 8 * c.ne,
                            hipMemcpyDeviceToHost));
    }
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
    HIP_CHECK(hipSetDevice(e->device));
    const int cap = max_phases >= 1 ? max_phases : kMaxPhases;
    auto *h = new mv_hierarchy;
    h->graphs.push_back(nullptr);
    h->maps.emplace_back();
    h->q.push_back(level_modularity(g));
    const mv_graph *cur = g;
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) {
        return std::chrono::duration<double, std::milli>(clk::now() - t0)
            .count();
    };
    for (int phase = 1; phase <= cap; phase++) {
        if (mv_engine_load_graph(e, cur) != 0) {
            delete h;
            return nullptr;
        }
        mv_phase_info pi{};
        pi.nv_in = e->lnv;
        pi.ne_in = e->lne;
        auto t0 = clk::now();
        pi.run_mod = mv_engine_run(e, lower, thresh, &pi.iters);
        pi.run_ms = ms_since(t0);
        h->info.push_back(pi);
        h->prop_nv.push_back(pi.nv_in);
        h->prop_q.push_back(h->q.back());
        mv_phase_info &info = h->info.back();

        // aggregate straight off the CSR the engine holds on the device
        t0 = clk::now();
        mv_coarse_dev c;
        if (mv_coarsen_device(e->stream, e->lnv, e->lne, e->d_xadj,
                              e->d_tails,
                              e->unit_weights ? nullptr : e->d_ew.get(),
                              phase_labels_device(e),
                              /*stop_if_identity*/ true, &c) != 0) {
            mv_coarse_dev_free(&c);
            delete h;
            return nullptr;
        }
        if (c.nc == e->lnv) { // no merge: the hierarchy is complete
            mv_coarse_dev_free(&c);
            break;
        }
        const double dev_ms = ms_since(t0); // the kernels, synchronised
        std::vector<i64> map(e->lnv), cx(c.nc + 1), ct(c.ne);
        std::vector<double> cw(c.ne);
        HIP_CHECK(hipMemcpy(map.data(), c.d_map, 8 * e->lnv,
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cx.data(), c.d_xadj, 8 * (c.nc + 1),
                            hipMemcpyDeviceToHost));
        if (c.ne) {
            HIP_CHECK(hipMemcpy(ct.data(), c.d_tails, 8 * c.ne,
                                hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(cw.data(), c.d_w, 8 * c.ne,
                                hipMemcpyDeviceToHost));
        }
        const double copy_ms = ms_since(t0) - dev_ms;
        const i64 parts[2] = {0, c.nc};
        mv_graph *ng = mv_graph_from_csr(c.nc, 0, 1, parts, c.nc, c.ne,
                                         cx.data(), ct.data(), cw.data());
        mv_coarse_dev_free(&c);
        info.coarsen_ms = ms_since(t0);
        if (getenv("MV_COARSEN_DEBUG"))
            std::fprintf(stderr,
                         "[coarsen] phase %d: device %.3f ms, D2H %.3f ms, "
                         "host level build %.3f ms\n",
                         phase, dev_ms, copy_ms,
                         info.coarsen_ms - dev_ms - copy_ms);
        if (!ng) {
            delete h;
            return nullptr;
        }
        const double qn = level_modularity(ng);
        h->prop_nv.back() = mv_graph_nv(ng);
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
    h->comm.resize(mv_graph_nv(g));
    for (size_t v = 0; v < h->comm.size(); v++) {
        i64 c = (i64)v;
        for (size_t k = 1; k < h->maps.size(); k++) c = h->maps[k][c];
        h->comm[v] = c;
    }
    return h;
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

mv_hierarchy *mv_engine_run_multiphase_dist(mv_engine *e, const mv_graph *g,
                                            double lower, double thresh,
                                            int max_phases) {
    HIP_CHECK(hipSetDevice(e->device));
    const int p = e->nranks;
    if (any_rank(e, slice_is_bad(e, g, "mv_engine_run_multiphase_dist")))
        return nullptr;
    const int cap = max_phases >= 1 ? max_phases : kMaxPhases;
    auto *h = new mv_hierarchy;
    h->graphs.push_back(nullptr);
    h->maps.emplace_back();
    h->q.push_back(level_modularity_dist(e, g));
    const mv_graph *cur = g;
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) {
        return std::chrono::duration<double, std::milli>(clk::now() - t0)
            .count();
    };
    std::vector<i64> mine(p), m((size_t)p * p);
    for (int phase = 1; phase <= cap; phase++) {
        // nv >= 2^31 is the one refusal of a load: global, so collective
        if (mv_engine_load_graph(e, cur) != 0) {
            delete h;
            return nullptr;
        }
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

        // aggregate straight off the slice the engine holds on the device
        t0 = clk::now();
        DistCoarse c;
        if (coarsen_dist_device(e, e->parts_h.data(), e->nv, e->lnv, e->lne,
                                e->d_xadj, e->d_tails,
                                e->unit_weights ? nullptr : e->d_ew.get(),
                                phase_labels_device(e), /*bad*/ false,
                                /*stop_if_identity*/ true, &c) != 0) {
            delete h;
            return nullptr;
        }
        if (c.nc == e->nv) break; // no merge anywhere: complete
        std::vector<i64> map(e->lnv);
        if (e->lnv)
            HIP_CHECK(hipMemcpy(map.data(), c.d_map, 8 * e->lnv,
                                hipMemcpyDeviceToHost));
        mv_graph *ng = level_from_device(e, c);
        info.coarsen_ms = ms_since(t0);
        if (any_rank(e, ng == nullptr)) {
            if (ng) mv_graph_free(ng);
            delete h;
            return nullptr;
        }
        const double qn = level_modularity_dist(e, ng);
        h->prop_nv.back() = c.nc;
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
    // final communities: one distributed lookup per kept level composes
    // the maps (level k's map is a table over level k-1's owners)
    const i64 lnv0 = mv_graph_lnv(g);
    h->comm.resize(lnv0);
    if (h->maps.size() == 1) {
        for (i64 v = 0; v < lnv0; v++)
            h->comm[v] = mv_graph_parts(g)[e->rank] + v;
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
    return h;
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
